"""The batches the hit-verification tests share (tests/test_verify_cpu.py, tests/test_gpu_verify.py): isoform-like random
transcriptomes of 40 transcripts of up to 900 bases (shared segments, N, lower case, transcripts shorter than k) whose reads -- 3 000
over the mapped cases, with 0 - 5 % substitutions, paired and single end -- are mapped by the restated scan contract
(oracle.mapper_oracle.scan_reads), and records made by hand for every mate status: positions wholly or partly off the transcript, a
read of 0 bases, reads of 1, 15, 16, 17, 63, 64, 65 and 257 bases, transcripts shorter than one 16-byte step.  Built once a process."""
import functools
import struct

import numpy as np

from oracle import mapper_oracle as MO
from oracle import oracle as O

COMP = bytes.maketrans(b"ACGTacgtN", b"TGCAtgcaN")
ACGT = np.frombuffer(b"ACGT", np.uint8)
EDGE_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 257)


def revcomp(s):
    return s.translate(COMP)[::-1]


def with_errors(rng, reads, rate):
    """substitutions at `rate` per base (A/C/G/T only; other characters stay)"""
    sub = {65: b"CGT", 67: b"AGT", 71: b"ACT", 84: b"ACG", 97: b"cgt", 99: b"agt", 103: b"act", 116: b"acg"}
    out = []
    for r in reads:
        b = bytearray(r)
        for i in np.nonzero(rng.random(len(b)) < rate)[0]:
            if b[i] in sub:
                b[i] = sub[b[i]][int(rng.integers(0, 3))]
        out.append(bytes(b))
    return out


def transcriptome(rng, M=40, k=31):
    base = rng.choice(ACGT, 4000)
    seqs = []
    for t in range(M):                                  # isoform-like: shared segments, so a seed occurs in several transcripts
        a = rng.integers(0, 3000); ln = rng.integers(k - 5, 900)
        s = base[a:a + ln].copy()
        if t % 7 == 0 and ln > 100:
            s[rng.integers(0, ln, 3)] = ord("N")
        if t % 5 == 0:
            s = np.frombuffer(s.tobytes().lower(), np.uint8)
        seqs.append(bytes(s))
    return seqs


def draw_reads(rng, seqs, n_reads, read_len):
    r1, r2 = [], []
    for _ in range(n_reads):
        s = seqs[rng.integers(0, len(seqs))]
        if len(s) < read_len + 20 or rng.random() < 0.05:
            r1.append(bytes(rng.choice(ACGT, rng.integers(10, read_len + 1)))); r2.append(r1[-1][::-1])      # noise / short reads
            continue
        frag = rng.integers(read_len, min(len(s), 300) + 1); p = rng.integers(0, len(s) - frag + 1)
        left = s[p:p + read_len]; right = revcomp(s[p + frag - read_len:p + frag])
        if rng.random() < 0.5:
            left, right = right, left
        if rng.random() < 0.1:
            left = left[:rng.integers(31, read_len)]     # ragged lengths: the mates' offsets are no multiples of 16
        if rng.random() < 0.05:
            b = bytearray(right); b[rng.integers(0, len(b))] = ord("N"); right = bytes(b)
        r1.append(bytes(left)); r2.append(bytes(right))
    return r1, r2


def _case(seqs, r1, r2, hits, off):
    return dict(seqs=seqs, r1=r1, r2=r2, hits=np.ascontiguousarray(hits, dtype=O.HIT_DTYPE), off=np.asarray(off, np.uint32))


def _mapped(seed, n_reads, read_len, rate, paired):
    rng = np.random.default_rng(seed)
    seqs = transcriptome(rng)
    r1, r2 = draw_reads(rng, seqs, n_reads, read_len)
    if rate:
        r1, r2 = with_errors(rng, r1, rate), with_errors(rng, r2, rate)
    hits, off = MO.scan_reads(MO.build_scan_index(seqs), r1, r2 if paired else None, s=19)
    return _case(seqs, r1, r2 if paired else None, hits, off)


def _edges(seed, paired):
    """records made by hand: every status of the library kind, every edge length, positions inside, partly off either end, wholly off"""
    rng = np.random.default_rng(seed)
    t0 = bytes(rng.choice(ACGT, 300))
    t2 = bytearray(rng.choice(ACGT, 40)); t2[7] = ord("N"); t2[20] = ord("n")
    seqs = [t0, t0[5:15], bytes(t2).lower(), t0[100:116], t0[:17], b"A", t0[30:290]]
    r1, r2, recs, off = [], [], [], [0]
    for L in EDGE_LENGTHS:
        for L2 in (EDGE_LENGTHS if paired else (0,) * 8):
            if paired and (L * 7 + L2) % 4 == 1:
                continue                                              # (a quarter of the 81 combinations less)
            src = bytes(rng.choice(ACGT, 20)) + t0 + bytes(rng.choice(ACGT, 20))
            p1, p2 = (int(rng.integers(0, max(1, len(src) - n + 1))) for n in (L, L2))
            m1, m2 = src[p1:p1 + L], revcomp(src[p2:p2 + L2])
            if rng.random() < 0.5:
                m1, m2 = revcomp(m1), revcomp(m2)
            m1, m2 = with_errors(rng, [m1, m2], 0.04)
            if L > 3 and rng.random() < 0.3:
                b = bytearray(m1); b[L // 2] = ord("N"); m1 = bytes(b)
            r1.append(m1); r2.append(m2)
            for _ in range(int(rng.integers(0, 6))):
                tid = int(rng.integers(0, len(seqs))); tl = len(seqs[tid])
                st = int(rng.integers(1, 4)) if paired else 0
                pos = [int(x) for x in rng.choice([-L - 3, -4, 0, p1 - 20, tl - L + 7, tl + 5, -1000, 1 << 20, int(rng.integers(-20, tl + 20))], 2)]
                if st == 2:
                    pos[0] = p2 - 20 if rng.random() < 0.5 else pos[0]
                fwd, mfwd = int(rng.integers(0, 2)), int(rng.integers(0, 2))
                a, b = (L2, L) if st == 2 else (L, L2)
                recs.append((tid, pos[0], pos[1] if st == 3 else 0, 0, a & 0xFFFF, b & 0xFFFF, fwd, mfwd if st == 3 else 0, st, 0))
            off.append(len(recs))
    return _case(seqs, r1, r2 if paired else None, np.array(recs, dtype=O.HIT_DTYPE), off)


def long_mate():
    """one mate of 70 000 bases against a transcript of 70 100: the loop over steps, saturating score fields, the 16-bit read_len"""
    rng = np.random.default_rng(5)
    t = bytes(rng.choice(ACGT, 70100))
    m = with_errors(rng, [t[60:70060]], 0.01)[0]
    far = b"N" * 70000                                                # every base a mismatch: mism saturates
    recs = [(0, 60, 0, 0, 70000 & 0xFFFF, 0, 1, 0, 0, 0), (0, 200, 0, 0, 70000 & 0xFFFF, 0, 0, 0, 0, 0), (1, -5, 0, 0, 70000 & 0xFFFF, 0, 1, 0, 0, 0),
            (0, 0, 0, 0, 70000 & 0xFFFF, 0, 1, 0, 0, 0), (0, -69000, 0, 0, 70000 & 0xFFFF, 0, 1, 0, 0, 0)]
    return _case([t, t[:50]], [m, revcomp(m), far], None, np.array(recs, dtype=O.HIT_DTYPE), [0, 1, 3, 5])


def clean_transcripts(rng, M=30):
    """isoform-like transcripts of A/C/G/T only (every fifth in lower case)"""
    base = rng.choice(ACGT, 3000)
    out = []
    for t in range(M):
        a = rng.integers(0, 2200); s = base[a:a + rng.integers(120, 800)].tobytes()
        out.append(s.lower() if t % 5 == 0 else s)
    return out


def planted_reads(rng, seqs, n):
    """random 100-base reads that carry one 25-base segment of a transcript (either strand) where a whole 31-mer starts: the scan
    contract finds the seed and reports the read"""
    reads = []
    for _ in range(n):
        s = seqs[rng.integers(0, len(seqs))]
        p = rng.integers(0, len(s) - 31 - 25); a = rng.integers(0, 76)
        seg = s[p:p + 25] if rng.random() < 0.5 else revcomp(s[p:p + 25])
        reads.append(bytes(rng.choice(ACGT, a)) + seg + bytes(rng.choice(ACGT, 75 - a)))
    return reads


def true_reads(rng, seqs, n, read_len=60):
    """error-free mates drawn wholly inside a transcript, from either strand -> (mate 1, mate 2)"""
    r1, r2 = [], []
    for _ in range(n):
        s = seqs[rng.integers(0, len(seqs))]
        frag = rng.integers(read_len, min(len(s), 250) + 1); p = rng.integers(0, len(s) - frag + 1)
        a, b = s[p:p + read_len], revcomp(s[p + frag - read_len:p + frag])
        if rng.random() < 0.5:
            a, b = b, a
        r1.append(a); r2.append(b)
    return r1, r2


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case (seqs, r1, r2 or None, hits, off); 3 000 mapped reads in all"""
    out = {
        "pe_clean": _mapped(11, 500, 70, 0.0, True),
        "pe_2pc": _mapped(12, 600, 70, 0.02, True),
        "pe_5pc": _mapped(13, 500, 100, 0.05, True),
        "se_clean": _mapped(14, 400, 70, 0.0, False),
        "se_3pc": _mapped(15, 600, 70, 0.03, False),
        "se_5pc": _mapped(16, 400, 50, 0.05, False),
        "edges_pe": _edges(21, True),
        "edges_se": _edges(22, False),
        "long": long_mate(),
    }
    assert sum(len(c["r1"]) for n, c in out.items() if n[2] == "_") == 3000
    return out


OPTIONS = [(p, kb) for p in (0, 900, 1000) for kb in (False, True)]


@functools.lru_cache(maxsize=None)
def expected(name, permille, keep_best):
    """verify_hits_host of a case: computed once, shared, never changed"""
    from sailfish_amd import hits as H
    c = cases()[name]
    h, o, s, st = H.verify_hits_host(c["seqs"], c["hits"], c["off"], c["r1"], c["r2"], permille, keep_best)
    for a in (h, o, s):
        a.setflags(write=False)
    return h, o, s, st


def packed(seqs):
    """list of bytes -> (the bytes back to back, uint64 offsets[n + 1])"""
    off = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return np.frombuffer(b"".join(seqs) + b"\0", np.uint8)[:-1].copy() if seqs else np.zeros(0, np.uint8), off


def blob(name, permille, keep_best):
    """a case with its expected result as the byte string tests/verify_harness.cpp's stand-alone program reads"""
    c = cases()[name]
    h, o, s, st = expected(name, permille, keep_best)
    ts, toff = packed(c["seqs"])
    s1, o1 = packed(c["r1"])
    s2, o2 = packed(c["r2"]) if c["r2"] is not None else (np.zeros(0, np.uint8), np.zeros(0, np.uint64))
    tl = np.array([len(x) for x in c["seqs"]], np.uint32)
    head = struct.pack("<11Q", len(c["seqs"]), len(ts), len(c["r1"]), len(s1), len(s2), len(c["hits"]), permille, int(keep_best),
                       int(c["r2"] is not None), len(h), 0)
    stats = np.array([st[k] for k in ("records_in", "records_out", "reads_in", "reads_out", "failed_identity", "dropped_not_best", "sum_mism")], np.uint64)
    parts = [ts, toff[:-1], tl, s1, o1, s2, o2, c["hits"], c["off"], h, o, s, stats]
    return head + b"".join(np.ascontiguousarray(p).tobytes() for p in parts)
