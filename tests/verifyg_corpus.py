"""The batches the gapped hit-verification tests share (tests/test_verifyg_cpu.py, tests/test_gpu_verifyg.py), about 2 000 reads:
mapped cases on verify_corpus.transcriptome with homopolymer-rich transcripts added (2 % substitutions, and in 30 % of the mates one
insertion or deletion of 1 - 4 bases at a uniform position, so before and behind the seeds), mapped by the restated scan contract;
records made by hand for every mate status (edge lengths, positions inside, near either end, partly and wholly off, transcripts
shorter than the band or than one window, N, lower case, both strands, indels of exactly k and of k + 1 bases, a pair with one mate
rescued and the other failing, a read with 70 records, reads without records); and one mate of 70 000 bases with three indels.  Built
once a process; the statement's edits are computed once per (case, k) and shared."""
import functools
import struct

import numpy as np

import verify_corpus as VC
from oracle import mapper_oracle as MO
from oracle import oracle as O

KS = (1, 2, 3, 7, 8, 15)
OPTIONS = [(p, kb) for p in (0, 900, 1000) for kb in (False, True)]
EDGE_LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 100, 257)
T = b"ACGTACGTAGCTAGCTAGGATCCATTGACCAGTTAGGCAT"            # 40 bases (tests/test_verify_cpu.py's)


def with_indel(rng, read, lo=1, hi=4):
    """one insertion (random bases) or deletion of lo .. hi bases at a uniform position"""
    n = int(rng.integers(lo, hi + 1))
    if len(read) <= n + 1:
        return read
    p = int(rng.integers(0, len(read) - n + 1))
    if rng.random() < 0.5:
        return read[:p] + bytes(rng.choice(VC.ACGT, n)) + read[p:]
    return read[:p] + read[p + n:]


def homopolymer_transcripts(rng, n=8):
    """transcripts of runs of 1 - 9 equal bases cut from one text: several optimal alignments tie in them"""
    runs = b"".join(bytes([int(rng.choice(VC.ACGT))]) * int(rng.integers(1, 10)) for _ in range(400))
    out = []
    for _ in range(n):
        a = int(rng.integers(0, len(runs) - 700))
        out.append(runs[a:a + int(rng.integers(200, 700))])
    return out


def _mapped(seed, n_reads, read_len, paired):
    rng = np.random.default_rng(seed)
    seqs = VC.transcriptome(rng) + homopolymer_transcripts(rng)
    r1, r2 = VC.draw_reads(rng, seqs, n_reads, read_len)
    r1, r2 = VC.with_errors(rng, r1, 0.02), VC.with_errors(rng, r2, 0.02)
    r1 = [with_indel(rng, r) if rng.random() < 0.3 else r for r in r1]
    r2 = [with_indel(rng, r) if rng.random() < 0.3 else r for r in r2]
    hits, off = MO.scan_reads(MO.build_scan_index(seqs), r1, r2 if paired else None, s=19)
    return VC._case(seqs, r1, r2 if paired else None, hits, off)


def _rec(tid, pos, st=0, fwd=1, mate_pos=0, mate_fwd=0, a=0, b=0):
    return (tid, pos, mate_pos if st == 3 else 0, 0, a & 0xFFFF, b & 0xFFFF, fwd, mate_fwd if st == 3 else 0, st, 0)


def _edges(seed, paired):
    """records made by hand: every status of the library kind, every edge length, positions inside, within the band of either end,
    partly off, wholly off; short transcripts; N and lower case in both texts"""
    rng = np.random.default_rng(seed)
    t0 = bytes(rng.choice(VC.ACGT, 400))
    t2 = bytearray(rng.choice(VC.ACGT, 60)); t2[7] = ord("N"); t2[20] = ord("n"); t2[21] = ord("N")
    seqs = [t0, t0[5:15], bytes(t2).lower(), t0[100:116], t0[:17], b"A", t0[30:390], t0[40:300].lower()]
    r1, r2, recs, off = [], [], [], [0]
    for L in EDGE_LENGTHS:
        for L2 in ((0, 2, 17, 33, 100) if paired else (0,) * 5):
            src = bytes(rng.choice(VC.ACGT, 20)) + t0 + bytes(rng.choice(VC.ACGT, 20))
            p1, p2 = (int(rng.integers(0, max(1, len(src) - n - 3))) for n in (L, L2))
            m1, m2 = src[p1:p1 + L + 4], src[p2:p2 + L2 + 4]          # (four bases more, so that an indel leaves the edge length whole)
            if L > 16 and rng.random() < 0.6:
                m1 = with_indel(rng, m1)
            if L2 > 16 and rng.random() < 0.6:
                m2 = with_indel(rng, m2)
            m1, m2 = m1[:L], VC.revcomp(m2[:L2])
            f1 = rng.random() < 0.5
            if not f1:
                m1, m2 = VC.revcomp(m1), VC.revcomp(m2)
            m1, m2 = VC.with_errors(rng, [m1, m2], 0.03)
            if L > 3 and rng.random() < 0.3:
                b = bytearray(m1); b[L // 2] = ord("N"); m1 = bytes(b)
            if rng.random() < 0.2:
                m1 = m1.lower()
            r1.append(m1); r2.append(m2)
            for _ in range(int(rng.integers(0, 6))):
                tid = int(rng.integers(0, len(seqs))); tl = len(seqs[tid])
                st = int(rng.integers(1, 4)) if paired else 0
                near = [p1 - 20, p1 - 20 + int(rng.integers(-3, 4)), p2 - 20, p2 - 20 + int(rng.integers(-3, 4))]
                pos = [int(x) for x in rng.choice(near + [-L - 3, -4, -1, 0, 1, 3, tl - L, tl - L + 2, tl - L + 7, tl - 1, tl + 5, -1000, 1 << 20,
                                                          int(rng.integers(-20, tl + 20))], 2)]
                if rng.random() < 0.5:                                # the true placement, on the transcript the mates come from
                    tid = 0
                    pos = [(p2 if st == 2 else p1) - 20, p2 - 20]
                    fwd, mfwd = (int(not f1) if st == 2 else int(f1)), int(not f1)
                else:
                    fwd, mfwd = int(rng.integers(0, 2)), int(rng.integers(0, 2))
                a, b = (L2, L) if st == 2 else (L, L2)
                recs.append(_rec(tid, pos[0], st, fwd, pos[1], mfwd, a, b))
            off.append(len(recs))
    return VC._case(seqs, r1, r2 if paired else None, np.array(recs, dtype=O.HIT_DTYPE), off)


def _indels(paired):
    """reads cut from one transcript with a deletion or an insertion of exactly k and of k + 1 bases in the middle, for every k of the
    grid, recorded on the diagonal of their first half (forward) or of their last half as the reverse strand sees it; a pair with one
    mate rescued and the other failing; a read with 70 records; reads without records"""
    rng = np.random.default_rng(77)
    t = bytes(rng.choice(VC.ACGT, 600))
    # a read with 2 bases deleted 8 from its end has two records: on t it costs its shifted tail ungapped and 2 edits with gaps; on a
    # copy of t that lacks the 2 bases and differs in 3 others it costs 3 either way -- keep_best keeps the copy's record ungapped
    # and drops it with gaps
    a0 = next(a for a in range(400, 500) if sum(x != y for x, y in zip(t[a + 54:a + 62], t[a + 52:a + 60])) >= 4)
    tail_read = t[a0:a0 + 52] + t[a0 + 54:a0 + 62]
    copy = bytearray(t[:a0 + 52] + t[a0 + 54:])
    for i in (a0 + 7, a0 + 21, a0 + 40):
        copy[i] = {65: 67, 67: 71, 71: 84, 84: 65}[copy[i]]
    seqs = [t, T, bytes(copy)]
    r1, r2, recs, off = [], [], [], [0]
    clean = VC.revcomp(t[300:400])

    def add(m1, m2, rr):
        r1.append(m1); r2.append(m2); recs.extend(rr); off.append(len(recs))
    for k in KS:
        for n in (k, k + 1):
            dele = t[100:150] + t[150 + n:200 + n]                    # 100 bases, n transcript bases skipped in the middle
            ins = t[100:150] + bytes(rng.choice(VC.ACGT, n)) + t[150:200]
            for m, shift in ((dele, n), (ins, -n)):                   # (the reverse records sit on the diagonal of the mate's far half)
                if paired:
                    add(m, clean, [_rec(0, 100, 3, 1, 300, 0, len(m), 100), _rec(0, 100, 1, 1, 0, 0, len(m), 100)])
                    add(clean, VC.revcomp(m), [_rec(0, 300, 3, 0, 100 + shift, 0, 100, len(m)), _rec(0, 100 + shift, 2, 0, 0, 0, len(m), 100)])
                else:
                    add(m, b"", [_rec(0, 100, 0, 1, a=len(m))])
                    add(VC.revcomp(m), b"", [_rec(0, 100 + shift, 0, 0, a=len(m))])
    mid2 = T[:20] + T[22:]                                            # the issue's first thing to look at, in small: 2 bases deleted
    add(mid2, VC.revcomp(mid2), [_rec(1, 0, 3, 1, 0, 0, 38, 38)] if paired else [_rec(1, 0, 0, 1, a=38)])
    if paired:                                                        # mate 1 is rescued by gaps, mate 2 matches nothing
        rescued = t[100:150] + t[152:202]
        add(rescued, bytes(rng.choice(VC.ACGT, 100)), [_rec(0, 100, 3, 1, 300, 0, 100, 100), _rec(0, 100, 1, 1, 0, 0, 100, 100)])
    many = t[200:260]
    st = 1 if paired else 0
    add(many, clean, [_rec(0, 200 + int(rng.integers(-6, 7)), st, 1, a=60) for _ in range(70)])
    add(tail_read, clean, [_rec(0, a0, st, 1, a=60), _rec(2, a0, st, 1, a=60)])
    for _ in range(3):
        add(bytes(rng.choice(VC.ACGT, 40)), bytes(rng.choice(VC.ACGT, 40)), [])
    add(many, clean, [_rec(0, 199, st, 1, a=60), _rec(0, 200, st, 1, a=60)])
    return VC._case(seqs, r1, r2 if paired else None, np.array(recs, dtype=O.HIT_DTYPE), off)


def long_mate():
    """one mate of 70 000 bases with 1 % substitutions and three indels against a transcript of 70 100, forward and as its reverse
    complement, and a mate of 70 000 N: the refill loop, saturating score fields, the 16-bit read_len"""
    rng = np.random.default_rng(6)
    t = bytes(rng.choice(VC.ACGT, 70100))
    m = VC.with_errors(rng, [t[60:70062]], 0.01)[0]
    m = (m[:9000] + m[9002:30000] + b"GAT" + m[30000:55000] + m[55001:])[:70000]      # 2 deleted at 9 000, 3 inserted at 30 000, 1 deleted at 55 000
    far = b"N" * 70000
    recs = [_rec(0, 60, 0, 1, a=70000), _rec(0, 60, 0, 0, a=70000), _rec(0, 0, 0, 1, a=70000)]
    return VC._case([t, t[:50]], [m, VC.revcomp(m), far], None, np.array(recs, dtype=O.HIT_DTYPE), [0, 1, 2, 3])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case (seqs, r1, r2 or None, hits, off)"""
    out = {
        "pe_indel": _mapped(51, 600, 70, True),
        "se_indel": _mapped(52, 700, 70, False),
        "edges_pe": _edges(61, True),
        "edges_se": _edges(62, False),
        "indels_pe": _indels(True),
        "indels_se": _indels(False),
        "long": long_mate(),
    }
    assert 1500 <= sum(len(c["r1"]) for c in out.values()) <= 2500
    return out


@functools.lru_cache(maxsize=None)
def edits(name, k):
    """gapped_edits_host of a case: computed once per (case, k), shared, never changed"""
    from sailfish_amd import hits as H
    c = cases()[name]
    e, u = H.gapped_edits_host(c["seqs"], c["hits"], c["off"], c["r1"], c["r2"], k)
    e.setflags(write=False); u.setflags(write=False)
    return e, u


@functools.lru_cache(maxsize=None)
def expected(name, k, permille, keep_best):
    """verify_hits_gapped_host of a case"""
    from sailfish_amd import hits as H
    c = cases()[name]
    h, o, s, st = H.verify_hits_gapped_host(c["seqs"], c["hits"], c["off"], c["r1"], c["r2"], permille, keep_best, k, edits=edits(name, k))
    for a in (h, o, s):
        a.setflags(write=False)
    return h, o, s, st


def blob(name, k, permille, keep_best):
    """a case with its expected result as the byte string tests/verifyg_harness.cpp's stand-alone program reads"""
    from sailfish_amd import hits as H
    c = cases()[name]
    h, o, s, st = expected(name, k, permille, keep_best)
    ts, toff = VC.packed(c["seqs"])
    s1, o1 = VC.packed(c["r1"])
    s2, o2 = VC.packed(c["r2"]) if c["r2"] is not None else (np.zeros(0, np.uint8), np.zeros(0, np.uint64))
    tl = np.array([len(x) for x in c["seqs"]], np.uint32)
    head = struct.pack("<11Q", len(c["seqs"]), len(ts), len(c["r1"]), len(s1), len(s2), len(c["hits"]), permille, int(keep_best),
                       int(c["r2"] is not None), len(h), k)
    stats = np.array([st[key] for key in H.VERIFYG_STATS], np.uint64)
    parts = [ts, toff[:-1], tl, s1, o1, s2, o2, c["hits"], c["off"], h, o, s, stats]
    return head + b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def check_coverage():
    """the corpus exercises the feature (asserted where it is built, on the CPU)"""
    from sailfish_amd import hits as H
    rescued = sum(expected(n, 3, 900, False)[3]["rescued"] for n in cases())
    assert rescued >= 50, rescued
    k3_not_k1 = mapped_never = best_drops = 0
    for n, c in cases().items():
        n_rec = len(c["hits"])
        lens = np.zeros((n_rec, 2), np.int64)
        for r in range(len(c["off"]) - 1):
            for i in range(c["off"][r], c["off"][r + 1]):
                st = int(c["hits"][i]["mate_status"])
                lens[i, 0] = len(c["r2"][r] if st == 2 else c["r1"][r])
                lens[i, 1] = len(c["r2"][r]) if st == 3 else 0
        ok = {k: np.all(1000 * (lens - edits(n, k)[0]) >= 900 * lens, axis=1) for k in KS}
        k3_not_k1 += int((ok[3] & ~ok[1]).sum())
        if n in ("pe_indel", "se_indel"):
            mapped_never += int((~np.any([ok[k] for k in KS], axis=0)).sum())
        if n != "long":                                               # keep_best at k = 3 drops a record that the ungapped keep_best keeps
            h0 = H.verify_hits_host(c["seqs"], c["hits"], c["off"], c["r1"], c["r2"], 900, True)[0]
            kept3, passing3 = (set(map(bytes, expected(n, 3, 900, kb)[0])) for kb in (True, False))
            best_drops += sum(1 for x in map(bytes, h0) if x in passing3 and x not in kept3)
    assert k3_not_k1 >= 10, k3_not_k1
    assert mapped_never >= 10, mapped_never
    assert best_drops >= 1, best_drops
    return dict(rescued=rescued, k3_not_k1=k3_not_k1, mapped_never=mapped_never, best_drops=best_drops)
