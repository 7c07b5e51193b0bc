"""Alignment batches as a mapper leaves them, for the BGZF and BAM writer tests (tests/test_bgzw_cpu.py, tests/test_bamwrite_cpu.py,
tests/test_gpu_bgzw.py, tests/test_gpu_bamwrite.py): reads
whose SEQ lengths agree with their records, 0 .. 8 records per read plus the odd 40, names of 1 .. 254 bytes, positions below
2^29 - 2^16.  `stream(paired, kind)` is what a writer of that format hands to the compressor: the SAM text of samfile._sam_text,
or sam_to_bam of it.  `corner` holds every rule of csrc/bamwfmt.h at its edges, `failing` the batches BAM cannot say.  A case is a dict
as in tests/samwrite_corpus.py."""
import functools

import numpy as np

from sailfish_amd.hits import HIT_DTYPE
from samwrite_corpus import rec

N_REFS = 400
POS_MAX = 2 ** 29 - 2 ** 16


def _transcripts():
    rng = np.random.default_rng(41)
    names = [b"ENST%011d.%d|ENSG%011d.%d" % (int(rng.integers(0, 10 ** 6)), int(rng.integers(1, 9)), int(rng.integers(0, 10 ** 5)), int(rng.integers(1, 9)))
             for _ in range(N_REFS)]
    ref_len = [int(x) for x in rng.integers(300, 20000, N_REFS)]
    ref_len[0] = 2 ** 29                                   # room for the largest position
    return names, ref_len


def case(paired, n_reads=3000, seed=0):
    rng = np.random.default_rng(4100 + seed + (1 if paired else 0))
    names, ref_len = _transcripts()
    bases = np.frombuffer(b"ACGT", np.uint8)
    hits, off, qnames, seqs = [], [0], [], []
    for r in range(n_reads):
        k = int(rng.integers(0, 9)) if rng.random() > 0.01 else 40
        rl, ml = int(rng.choice([50, 75, 100, 100, 100, 151])), int(rng.choice([50, 75, 100, 100, 100, 151]))
        if r % 1000 == 7:
            qnames.append(b"Q" * (1 if r < 1000 else 254))
        else:
            qnames.append(b"SRR%d.%d" % (1234567 + seed, r + 1) + (b" length=%d" % rl if r % 3 == 0 else b""))
        s1, s2 = rng.choice(bases, rl).tobytes(), rng.choice(bases, ml).tobytes()
        seqs.append((s1, s2) if paired else s1)
        for _ in range(k):
            tid = int(rng.integers(0, N_REFS))
            top = POS_MAX if tid == 0 else ref_len[tid]
            pos = int(rng.integers(0, top))
            if paired:
                status = int(rng.choice([3, 3, 3, 3, 1, 2]))
                frag = int(rng.integers(max(rl, ml), 600))
                fwd = int(rng.integers(0, 2))
                if status == 3:
                    hits.append((tid, pos, pos + frag - ml, frag, rl, ml, fwd, 1 - fwd, 3, 0))
                else:
                    hits.append((tid, pos, 0, 0, rl if status == 1 else ml, 0, fwd, 0, status, 0))
            else:
                hits.append((tid, pos, 0, 0, rl, 0, int(rng.integers(0, 2)), 0, 0, 0))
        off.append(len(hits))
    return dict(names=names, ref_len=ref_len, hits=np.array(hits, HIT_DTYPE), offsets=np.array(off, np.uint32), paired=paired,
                read_names=qnames, seqs=seqs)


@functools.lru_cache(maxsize=None)
def stream(paired, kind, n_reads=3000):
    """bytes handed to the compressor for the corpus: kind 'sam' (the text, header lines included) or 'bam' (the BAM stream)"""
    from sailfish_amd import samfile
    c = case(paired, n_reads)
    text = samfile._sam_text(c["names"], c["ref_len"], c["hits"], c["offsets"], c["read_names"], c["seqs"])
    return text if kind == "sam" else samfile.sam_to_bam(text)


# [beg, beg + 50) lies in one bin of 16 KB, then crosses a border of 2^14, 2^17, 2^20, 2^23 and 2^26: the five levels and bin 0
BIN_STARTS = [100, 2 ** 14 - 10, 2 ** 17 - 10, 2 ** 20 - 10, 2 ** 23 - 10, 2 ** 26 - 10]
BIN_WANT = [4681, 585, 73, 9, 1, 0]
ODD_BASES = bytes(range(33, 256))                          # lower case, every IUPAC letter, '=', and bytes that are no base: 223 of them


def _case(paired, reads):
    names, ref_len = _transcripts()
    hits = np.array([r for _, _, recs in reads for r in recs], HIT_DTYPE)
    off = np.concatenate([[0], np.cumsum([len(recs) for _, _, recs in reads])]).astype(np.uint32)
    return dict(names=names, ref_len=ref_len, hits=hits, offsets=off, paired=paired, read_names=[q for q, _, _ in reads],
                seqs=[s for _, s, _ in reads])


def corner(paired, long_seqs=(9000,)):
    """every branch of SamwLine and every rule of csrc/bamwfmt.h at its edges, with SEQ lengths that agree with the records;
    long_seqs: the lengths of the long SEQs (one read each)"""
    rng = np.random.default_rng(11)
    seq = lambda n: bytes(rng.choice(np.frombuffer(b"ACGTNacgtnRYKMSWBDHV=", np.uint8), n).tobytes())
    top = 2 ** 29
    reads = []
    if paired:
        P = lambda tid, pos, mpos, rl, ml, frag=200, fwd=1, mfwd=0: rec(tid, pos, mpos, frag, rl, ml, fwd, mfwd, 3)
        O = lambda tid, pos, status, n, fwd=1: rec(tid, pos, 0, 0, n, 0, fwd, 0, status)
        sq = lambda a, b: (seq(a), seq(b))
        reads += [(b"none", sq(100, 99), []),
                  (b"one", sq(50, 60), [P(1, 10, 150, 50, 60)]),
                  (b"three", sq(50, 60), [P(1, 7, 7, 50, 60, 50), P(2, 300, 100, 50, 60, 250, 0, 1), P(5, 100, 300, 50, 60, 250, 0, 0)]),
                  (b"strands", sq(1, 2), [P(3, 1, 2, 1, 2, 3, f, m) for f in (0, 1) for m in (0, 1)]),
                  (b"orph", sq(50, 61), [O(1, 5, 1, 50), O(3, 6, 1, 50, 0), O(7, 0, 2, 61), O(4, 2, 2, 61, 0)]),
                  (b"clip", sq(50, 60), [P(3, -49, -59, 50, 60, 60), P(3, 0, -59, 50, 60, 109), O(3, -49, 1, 50), O(3, -1, 2, 60, 0)]),
                  (b"Q", sq(48, 49), [P(6, 20, 40, 48, 49)]),
                  (b"Q" * 254, sq(49, 48), [P(6, 20, 40, 49, 48), O(6, 1, 2, 48)]),
                  (b"name with spaces", sq(1, 0), []),
                  (b"odd", (ODD_BASES, ODD_BASES[::-1]), [P(8, 5, 50, 223, 223), O(8, 9, 1, 223)]),
                  (b"len", sq(1, 65535), [P(0, 0, 0, 1, 65535, 1), P(0, 0, -65534, 1, 65535, 1), O(0, top - 2 ** 16, 2, 65535)]),
                  (b"len2", sq(65535, 1), [O(0, -65534, 1, 65535), P(0, top - 2 ** 16, top - 1, 65535, 1, 65535)]),
                  (b"end", sq(50, 50), [P(0, top - 50, top - 2 ** 16, 50, 50, 2 ** 16)])]
        reads += [(b"bin%d" % i, sq(50, 50), [P(0, b, BIN_STARTS[-1 - i], 50, 50), O(0, b, 1 + i % 2, 50)]) for i, b in enumerate(BIN_STARTS)]
        reads += [(b"long%d" % n, sq(n, 1), [P(0, 1, 2, n, 1)]) for n in long_seqs]
        reads += [(b"longnone", sq(3, long_seqs[0]), [])]
    else:
        S = lambda tid, pos, n, fwd=1: rec(tid, pos, 0, 0, n, 0, fwd, 0, 0)
        reads += [(b"none", seq(100), []),
                  (b"one", seq(50), [S(1, 10, 50)]),
                  (b"three", seq(50), [S(1, 7, 50, 0), S(2, 300, 50), S(5, 100, 50, 0)]),
                  (b"clip", seq(50), [S(1, 0, 50), S(1, -1, 50), S(1, -49, 50)]),
                  (b"Q", seq(48), [S(6, 20, 48)]),
                  (b"Q" * 254, seq(49), [S(6, 20, 49, 0)]),
                  (b"name with spaces", seq(0), []),
                  (b"odd", ODD_BASES, [S(8, 5, 223)]),
                  (b"len", seq(1), [S(0, 0, 1), S(0, top - 2 ** 16, 1, 0)]),
                  (b"len2", seq(65535), [S(0, 0, 65535), S(0, -65534, 65535), S(0, top - 2 ** 16, 65535, 0)]),
                  (b"end", seq(50), [S(0, top - 50, 50)])]
        reads += [(b"bin%d" % i, seq(50), [S(0, b, 50, i & 1)]) for i, b in enumerate(BIN_STARTS)]
        reads += [(b"long%d" % n, seq(n), [S(0, 1, n)]) for n in long_seqs]
        reads += [(b"longnone", seq(long_seqs[0]), [])]
    return _case(paired, reads)


def failing(paired):
    """[(case, read, record, kind)]: batches BAM cannot say and the lowest offender -- kind 3 the read name, 4 the number of bases,
    5 the end of the alignment (csrc/bamwfmt.h), behind samwfmt.h's kinds 1 (position) and 2 (tid) where one record breaks several.
    A read without records counts as record 0.  Every case carries names and bases."""
    st, top = (3 if paired else 0), 2 ** 29
    R = lambda tid, pos, n=4: rec(tid, pos, pos if paired else 0, n if paired else 0, n, n if paired else 0, 1, 0, st)
    ok, far, no_tid, no_base = R(1, 5), R(0, top - 3), R(N_REFS, 5), R(1, -4)
    s4, s5 = ((b"ACGT", b"TTGA") if paired else b"ACGT"), ((b"ACGTA", b"TTGA") if paired else b"ACGTA")
    mate = (b"ACGT", b"TTG") if paired else b"ACG"
    mk = lambda reads: _case(paired, reads)
    return [(mk([(b"a", s4, [ok]), (b"b", s4, []), (b"", s4, [ok, ok]), (b"d", s5, [ok])]), 2, 0, 3),
            (mk([(b"a", s4, [ok]), (b"Q" * 255, s4, []), (b"", s4, [ok])]), 1, 0, 3),
            (mk([(b"a", s4, [ok, ok, ok]), (b"b", s5, [ok]), (b"", s4, [ok])]), 1, 0, 4),
            (mk([(b"a", s4, [ok]), (b"b", mate, [ok, ok])]), 1, 0, 4),
            (mk([(b"a", s4, [ok]), (b"b", (s4[0] if paired else s4) * 16384, [])] if not paired else
                [(b"a", s4, [ok]), (b"b", (b"A", b"ACGT" * 16384), [])]), 1, 0, 4),
            (mk([(b"a", s4, [ok, far]), (b"", s4, [ok])]), 0, 1, 5),
            (mk([(b"a", s4, [ok] * 300 + [far]), (b"", s5, [far])]), 0, 300, 5),
            (mk([(b"", s5, [far])]), 0, 0, 3),                                   # one record breaking 3, 4 and 5
            (mk([(b"a", s5, [far])]), 0, 0, 4),                                  # 4 and 5
            (mk([(b"", s5, [no_tid])]), 0, 0, 2),                                # samwfmt.h's rules come first
            (mk([(b"", s5, [ok, no_base])]), 0, 0, 3),                           # ... but the lowest (read, record) before any kind
            (mk([(b"a", s4, [ok, no_base]), (b"", s4, [])]), 0, 1, 1)]
