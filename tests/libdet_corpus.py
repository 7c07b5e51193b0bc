"""The batches the library-format tests share (tests/test_libdet_cpu.py, tests/test_gpu_libdet.py): one synthetic batch of about
3 000 reads without real bases -- reads of every kind, mixed reads, the max_read_occs edge, one read long enough to take its block off
the LDS stage, the hitType edges -- whose second part keeps the mapper's contract (all pairs, or a left-orphan run then a right-orphan
run, or all single-end) so that the hit filter can be held against it; and six simulated protocols over tests/rescue_corpus.py's
spliced transcriptome.  Built once a process."""
import functools

import numpy as np

import rescue_corpus as RC

KINDS = ("ISF", "ISR", "OSF", "OSR", "MSF", "MSR", "LF", "LR", "RF", "RR", "SF", "SR", "other")
STATS = ("reads", "reads_mapped", "reads_over_occs", "reads_mixed", "reads_compatible", "votes", "records_kind", "reads_kind", "votes_kind")
FORMATS = ("IU", "ISF", "ISR", "OU", "OSF", "OSR", "MU", "MSF", "MSR", "U", "SF", "SR")
MAX_READ_OCCS = 40                      # (small, so that the edge reads stay small)
LONG_READ = 2000                        # records: more than the kernel's stage of 1536
HIT_DTYPE = np.dtype([("tid", "<u4"), ("pos", "<i4"), ("mate_pos", "<i4"), ("frag_len", "<u4"), ("read_len", "<u2"),
                      ("mate_len", "<u2"), ("fwd", "u1"), ("mate_fwd", "u1"), ("mate_status", "u1"), ("pad_", "u1")])


def rec(kind, tid=0, pos=100, length=50):
    """a record of the named kind, far from every edge"""
    if kind in ("ISF", "ISR", "OSF", "OSR"):
        f1 = kind[2] == "F"
        inward = kind[0] == "I"
        fwd_pos, rev_pos = (pos, pos + 150) if inward else (pos + 150, pos)          # the forward mate lies upstream iff inward
        p1, p2 = (fwd_pos, rev_pos) if f1 else (rev_pos, fwd_pos)
        return (tid, p1, p2, 200, length, length, int(f1), int(not f1), 3, 0)
    if kind in ("MSF", "MSR"):
        f = int(kind == "MSF")
        return (tid, pos, pos + 150, 200, length, length, f, f, 3, 0)
    if kind == "other":
        return (tid, pos, 0, 0, length, 0, 1, 0, 4 + tid % 250, 0)
    status = {"L": 1, "R": 2, "S": 0}[kind[0]]
    return (tid, pos, 0, 0, length, 0, int(kind[1] == "F"), 0, status, 0)


def pair(p1, l1, f1, p2, l2, f2):
    return (7, p1, p2, 0, l1, l2, f1, f2, 3, 0)


# the hitType edges: (record, kind without dovetailing, kind with); s1 / s2 are pos (forward) or pos + len (reverse)
EDGES = [
    (pair(100, 50, 1, 50, 50, 0), "ISF", "ISF"),                       # s1 == s2 (= 100)
    (pair(101, 50, 1, 50, 50, 0), "OSF", "ISF"),                       # s1 == s2 + 1
    (pair(150, 50, 1, 50, 50, 0), "OSF", "ISF"),                       # s1 == s2 + len2: the last dovetail
    (pair(151, 50, 1, 50, 50, 0), "OSF", "OSF"),                       # ... + 1
    (pair(50, 50, 0, 100, 50, 1), "ISR", "ISR"),                       # mirrored: s2 == s1
    (pair(50, 50, 0, 101, 50, 1), "OSR", "ISR"),
    (pair(50, 60, 0, 170, 50, 1), "OSR", "ISR"),                       # s2 == s1 + len1 (s1 = 110)
    (pair(50, 60, 0, 171, 50, 1), "OSR", "OSR"),
    (pair(-30, 50, 1, -60, 50, 0), "ISF", "ISF"),                      # negative positions: s1 = -30, s2 = -10
    (pair(-30, 50, 1, -80, 50, 0), "ISF", "ISF"),                      # s1 = -30 == s2
    (pair(-29, 50, 1, -80, 50, 0), "OSF", "ISF"),
    (pair(-5, 50, 0, -20, 50, 1), "ISR", "ISR"),                       # s1 = 45, s2 = -20
    (pair(2 ** 31 - 20, 50, 0, 10, 50, 1), "OSR", "OSR"),              # pos + len wraps in uint32: s1 = -2^31 + 30, far below s2
    (pair(10, 50, 1, 2 ** 31 - 20, 50, 0), "OSF", "OSF"),              # the mate's sum wraps: s2 = -2^31 + 30, s1 above it
    (pair(2 ** 31 - 20, 50, 1, 2 ** 31 - 60, 50, 0), "ISF", "ISF"),    # s2 = 2^31 - 10 does not wrap; s2 + stretch is taken in 64 bits
    (pair(-2 ** 31, 50, 1, 2 ** 31 - 1, 0, 0), "ISF", "ISF"),          # the extremes: s1 = -2^31, s2 = 2^31 - 1
    (pair(2 ** 31 - 1, 65535, 1, 2 ** 31 - 1, 65535, 1), "MSF", "MSF"),
    (pair(0, 0, 0, 0, 0, 0), "MSR", "MSR"),
]


@functools.lru_cache(maxsize=None)
def batch():
    """-> (hits HIT_DTYPE, offsets uint32[R + 1], first read of the contract-abiding part, first record of it)"""
    rng = np.random.default_rng(1303)
    recs, off = [], [0]

    def read(rs):
        recs.extend(rs); off.append(len(recs))

    # ---- part 1: anything goes --------------------------------------------------------------------------------------------------
    for k in KINDS:                                                      # one-record reads of each kind, reads without records between
        read([rec(k)]); read([])
    for r, _, _ in EDGES:
        read([r])
    read([rec("ISF"), rec("ISR")]); read([rec("LF"), rec("ISF")]); read([rec("SF"), rec("SR"), rec("SF")])          # mixed
    read([rec("other"), rec("ISF")]); read([rec(k, tid=i) for i, k in enumerate(KINDS)]); read([rec("MSF")] * 3 + [rec("MSR")])
    read([rec("ISF", tid=i) for i in range(MAX_READ_OCCS)]); read([rec("ISF", tid=i) for i in range(MAX_READ_OCCS + 1)])
    read([rec("SR", tid=i) for i in range(MAX_READ_OCCS)] + [rec("SF")]); read([rec("ISR", tid=i) for i in range(MAX_READ_OCCS - 1)] + [rec("OSR")])
    for _ in range(700):                                                 # random reads, most of one kind
        n = int(rng.choice([0, 1, 1, 1, 2, 3, 5, 9]))
        if rng.random() < 0.8:
            k = KINDS[int(rng.integers(0, 13))]
            read([rec(k, tid=int(rng.integers(0, 500)), pos=int(rng.integers(-40, 3000))) for _ in range(n)])
        else:
            read([rec(KINDS[int(rng.integers(0, 13))], tid=int(rng.integers(0, 500))) for _ in range(n)])
    for _ in range(300):                                                 # random pairs around the inward / outward boundary
        l1, l2 = int(rng.integers(0, 120)), int(rng.integers(0, 120))
        p1 = int(rng.integers(-100, 400))
        read([pair(p1, l1, int(rng.integers(0, 2)), p1 + int(rng.integers(-130, 131)), l2, int(rng.integers(0, 2))) for _ in range(int(rng.integers(1, 3)))])
    read([rec("ISF", tid=i) for i in range(LONG_READ)])                  # over max_read_occs, and its block leaves the LDS stage
    for _ in range(260):
        read([rec("ISR")])
    # ---- part 2: the mapper's contract ------------------------------------------------------------------------------------------
    first_read, first_rec = len(off) - 1, len(recs)
    pairs, lefts, rights, singles = KINDS[:6], KINDS[6:8], KINDS[8:10], KINDS[10:12]
    for _ in range(1700):
        shape, n = rng.random(), int(rng.choice([0, 1, 1, 1, 2, 2, 3, 6]))
        tids = sorted(int(t) for t in rng.integers(0, 500, n))
        if shape < 0.5:                                                  # all pairs; mostly of one kind
            k = pairs[int(rng.integers(0, 6))]
            read([rec(k if rng.random() < 0.85 else pairs[int(rng.integers(0, 6))], tid=t, pos=int(rng.integers(0, 2000))) for t in tids])
        elif shape < 0.8:                                                # a left-orphan run, then a right-orphan run, each ascending in tid
            cut = int(rng.integers(0, n + 1))
            read([rec(lefts[int(rng.integers(0, 2))], tid=t) for t in sorted(tids[:cut])] + [rec(rights[int(rng.integers(0, 2))], tid=t) for t in sorted(tids[cut:])])
        else:
            read([rec(singles[int(rng.integers(0, 2))], tid=t) for t in tids])
    read([rec("ISF", tid=i) for i in range(MAX_READ_OCCS + 1)]); read([rec("OSR", tid=i) for i in range(MAX_READ_OCCS)])
    hits = np.array(recs, dtype=HIT_DTYPE)
    offsets = np.array(off, np.uint32)
    hits.setflags(write=False); offsets.setflags(write=False)
    return hits, offsets, first_read, first_rec


def abiding():
    """the contract-abiding part as a batch of its own"""
    h, o, r0, h0 = batch()
    return h[h0:], (o[r0:] - h0).astype(np.uint32)


def n_voters(paired, dovetail=False):
    return expected(paired, dovetail, 1 << 40)[1]["votes"]


def splits():
    """how the tests cut the batch into calls: at once, and 100 reads a call"""
    R = len(batch()[1]) - 1
    return [[(0, R)], [(a, min(a + 100, R)) for a in range(0, R, 100)]]


def budgets(paired, dovetail=False):
    """remaining_votes: none, one, one that ends inside a block, exactly the voters, more"""
    v = n_voters(paired, dovetail)
    return [0, 1, 150, v, v + 5]


def slice_batch(h, o, a, b):
    return h[o[a]:o[b]], (o[a:b + 1] - o[a]).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def expected(paired, dovetail, budget, expected_format=None):
    """library_kinds_host over the whole batch: computed once, shared, never changed"""
    from sailfish_amd import hits as H
    h, o, _, _ = batch()
    return H.library_kinds_host(h, o, paired_library=paired, max_read_occs=MAX_READ_OCCS, allow_dovetail=dovetail, remaining_votes=budget, expected=expected_format)


def stats_vector(st):
    """the stats dict in the layout of sfgpu_libdet_stats: 6 + 3 * 13 uint64"""
    return np.array([st[k] for k in STATS[:6]] + [v for k in STATS[6:] for v in st[k]], np.uint64)


# ---- simulated libraries -------------------------------------------------------------------------------------------------------------
PROTOCOLS = ("ISF", "ISR", "IU", "SF", "SR", "U")
SIM_SEED, SIM_READS, SIM_LEN, SIM_RATE = 11, 400, 50, 0.02


@functools.lru_cache(maxsize=None)
def simulated(protocol, seed=SIM_SEED):
    """400 reads of 50 bases with 2 % substitutions from the spliced transcriptome, made by the named protocol: fragments of about 250
    bases whose mate 1 is the sense end (ISF), the antisense end (ISR) or either (IU); single-end reads that are sense (SF), antisense
    (SR) or either (U).  -> (names, transcripts, reads 1, reads 2 or None)"""
    rng = np.random.default_rng(seed)
    seqs = RC.spliced_transcriptome(rng)
    r1, r2 = [], []
    while len(r1) < SIM_READS:
        s = seqs[int(rng.integers(0, len(seqs)))]
        frag = max(SIM_LEN, int(round(rng.normal(250, 25))))
        if frag > len(s):
            continue
        p = int(rng.integers(0, len(s) - frag + 1))
        sense, anti = s[p:p + SIM_LEN], RC.revcomp(s[p + frag - SIM_LEN:p + frag])
        flip = {"ISF": False, "SF": False, "ISR": True, "SR": True}.get(protocol, rng.random() < 0.5)
        a, b = (anti, sense) if flip else (sense, anti)
        r1.append(a); r2.append(b)
    r1 = RC.with_errors(rng, r1, SIM_RATE)
    r2 = RC.with_errors(rng, r2, SIM_RATE) if protocol in ("ISF", "ISR", "IU") else None
    return ["tx%d" % i for i in range(len(seqs))], seqs, r1, r2


def blob_cases():
    """what the stand-alone harness runs: (paired, dovetail, expected format or None, budget, reads per call)"""
    R = len(batch()[1]) - 1
    return [(True, False, None, n_voters(True) + 5, R), (True, True, "ISF", 150, 100), (False, False, "SR", 1, 100), (True, False, "OU", 0, 256),
            (False, True, "U", n_voters(False, True), 1)]


def blob():
    """the batch and the statement's counters for blob_cases(), as the byte string tests/libdet_harness.cpp's stand-alone program reads"""
    from sailfish_amd import hits as H
    h, o, _, _ = batch()
    cases = blob_cases()
    parts = [np.array([len(o) - 1, len(h), len(cases)], np.uint64), h, o]
    for paired, dovetail, fmt, budget, per_call in cases:
        rem, st = expected(paired, dovetail, budget, fmt)
        t = H.LIBRARY_FORMATS[fmt] if fmt else (0, 0, 0)
        parts += [np.array([MAX_READ_OCCS, paired, dovetail, fmt is not None, *t, budget, per_call], np.uint64), stats_vector(st), np.array([rem], np.uint64)]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)
