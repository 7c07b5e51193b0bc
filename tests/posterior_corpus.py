"""What the posterior tests share (tests/test_posterior_cpu.py, tests/test_gpu_posterior.py): the weight table and the reads of the
pass's corpus -- every size at which the lane groups of csrc/posterior.hip or the tree of csrc/postfmt.h change shape, and the special
reads of the rule -- with the statement's result, computed once; the small writable batches, cut from tests/mdtag_corpus.py, with
values for the writers to place; and the end-to-end reads over the spliced transcriptome of tests/rescue_corpus.py."""
import functools
import struct

import numpy as np

from oracle import oracle as O

N_REFS = 50
GENERAL = 40                                  # transcripts 0 .. 39 carry the random weights; the rest are the special ones below
SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 1000)
READS_PER_SIZE = 20
ZERO, TINY, ONE, THREE, TWO, HUGE, SMALL = 46, 47, 40, 41, 42, 48, 49
STATS = ("reads", "reads_mapped", "reads_multi", "records", "reads_flat", "records_zero", "max_records")
# (name, the read's tids, what the tokens must be or None)
SPECIAL = (
    ("all_zero", [ZERO, 3, TINY], ["0.333333"] * 3),                  # every weight 0 or read as 0: spread evenly
    ("below_tiny", [TINY, ONE], ["0", "1"]),                          # 2^-1000 reads as 0
    ("flushed", [HUGE, SMALL, SMALL], ["1", "0", "0"]),              # 10^40 apart: below 2^-56
    ("twice", [ONE, ONE, TWO], ["0.25", "0.25", "0.5"]),             # a transcript with two records has two terms
    ("quarter", [ONE, THREE], ["0.25", "0.75"]),
    ("third", [ONE, TWO], ["0.333333", "0.666667"]),
    ("seventh", [ONE] * 7, ["0.142857"] * 7),
    ("alone_zero", [ZERO], ["1"]),
)


@functools.lru_cache(maxsize=None)
def weights():
    rng = np.random.default_rng(36)
    w = np.zeros(N_REFS, np.float64)
    w[:GENERAL] = 10.0 ** rng.uniform(-8, 8, GENERAL)
    w[[3, 17]] = 0.0
    w[30] = 2.0 ** -961                       # a normal number below the rule's 2^-960
    w[ONE], w[THREE], w[TWO] = 1.0, 3.0, 2.0
    w[ZERO], w[TINY], w[HUGE], w[SMALL] = 0.0, 2.0 ** -1000, 1e30, 1e-10
    w.setflags(write=False)
    return w


def records(tids):
    h = np.zeros(len(tids), O.HIT_DTYPE)
    h["tid"] = tids
    h["read_len"], h["fwd"] = 20, 1
    return h


@functools.lru_cache(maxsize=None)
def batch():
    """-> (hits, offsets uint32[R + 1], size class of every read (-1: a special read), the names of the special reads by read)"""
    rng = np.random.default_rng(37)
    tids, off, cls, special = [], [0], [], {}
    for rep in range(READS_PER_SIZE):
        for n in SIZES:                       # the sizes interleaved, so that a block of 256 reads holds every width class
            if n == 0 and rep >= 3:
                continue
            tids.extend(rng.integers(0, GENERAL, n).tolist())
            off.append(len(tids)); cls.append(n)
        if rep < len(SPECIAL):
            name, t, _ = SPECIAL[rep]
            special[len(cls)] = name
            tids.extend(t); off.append(len(tids)); cls.append(-1)
    h, o = records(tids), np.asarray(off, np.uint32)
    h.setflags(write=False); o.setflags(write=False)
    return h, o, np.asarray(cls), special


@functools.lru_cache(maxsize=None)
def expected():
    """posteriors_host of the batch: (p, rec, f32, stats), computed once, shared, never changed"""
    from sailfish_amd import hits as H
    h, o, _, _ = batch()
    p, rec, f32, st = H.posteriors_host(h, o, weights())
    for a in (p, rec, f32):
        a.setflags(write=False)
    return p, rec, f32, st


def tokens(p):
    return ["%g" % v for v in np.asarray(p).tolist()]


def blob():
    """the batch with its expected result as the byte string tests/posterior_harness.cpp's stand-alone program reads"""
    h, o, _, _ = batch()
    p, rec, f32, st = expected()
    head = struct.pack("<3Q", len(o) - 1, len(h), N_REFS)
    parts = [np.ascontiguousarray(h), o, weights(), p, rec, f32, np.array([st[k] for k in STATS], np.uint64)]
    return head + b"".join(np.ascontiguousarray(a).tobytes() for a in parts)


# ---- the writable batches ----------------------------------------------------------------------------------------------------------

WRITER_CASES = ("runs_se", "runs_pe", "ag_se_indel_aligned", "ag_pe_indel_aligned")
WRITER_READS = 40


def cut(case, aln, tags, R):
    """the first R reads of a case of tests/mdtag_corpus.py with their alignment and tags"""
    R = min(R, len(case["r1"]))
    n = int(case["off"][R])
    c = dict(seqs=case["seqs"], r1=case["r1"][:R], r2=None if case["r2"] is None else case["r2"][:R], hits=case["hits"][:n], off=case["off"][:R + 1].copy())
    if aln is not None:
        pos, nm, op_off, ops = aln[:4]
        aln = (pos[:2 * n], nm[:2 * n], op_off[:2 * n + 1], ops[:int(op_off[2 * n])])
    if tags is not None:
        nm, md_off, md = tags[:3]
        tags = (nm[:2 * n], md_off[:2 * n + 1], md[:int(md_off[2 * n])])
    return c, aln, tags


def values(n, seed=38):
    """what hits.posteriors_host leaves for n records whose values are made up -- the writers only place them: 0, 1, the short and
    the long tokens, the smallest value the rule writes, and 10^U(-17, 0) -> (p, rec, f32)"""
    from sailfish_amd import hits as H
    rng = np.random.default_rng(seed)
    fixed = [0.0, 1.0, 0.5, 1 / 3, 2 / 3, 1.234567e-05, 2.0 ** -56, 0.9999995, 9.99999e-05, 0.0001]
    p = np.array([fixed[i % len(fixed)] if i % 3 == 0 else 10.0 ** rng.uniform(-17, 0) for i in range(n)], np.float64)
    p[p < 2.0 ** -56] = 0.0
    return p, np.array([H.posterior_record(v) for v in p.tolist()], np.uint32), np.array([float("%g" % v) for v in p.tolist()], np.float64).astype(np.float32)


def quals(reads):
    """quality bytes for every read: '!' .. '~', differing along the read"""
    return [bytes(33 + (7 * i + 3 * j) % 94 for j in range(len(r))) for i, r in enumerate(reads)]


@functools.lru_cache(maxsize=None)
def writable(name):
    """-> (case, alignment or None, tags, (p, rec, f32) for the case's records): about WRITER_READS reads"""
    import mdtag_corpus as MC
    c, aln, tags = cut(*MC.writable(name), WRITER_READS)
    return c, aln, tags, values(len(c["hits"]))


TOKENS_AT_THE_EDGE = ("1", "0.333333", "1.23457e-05")


def qnames_case(first_name_len, token):
    """tests/mdtag_corpus.py's batch whose first QNAME is first_name_len bytes long, with a posterior per record whose token is `token`
    -> (case, read names, (p,))"""
    import mdtag_corpus as MC
    case, names = MC.qnames_case(first_name_len)
    p = np.full(len(case["hits"]), float(token), np.float64)
    assert "%g" % p[0] == token if len(p) else True
    return case, names, p


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

E2E_READS, E2E_BATCH = 600, 200


def end_to_end():
    """names, transcripts, mate 1 and mate 2 of 600 pairs over the spliced transcriptome: most reads hit several isoforms"""
    import rescue_corpus as RC
    names, seqs, r1, r2, _ = RC.end_to_end(n=E2E_READS)
    return names, seqs, r1, r2
