"""The batches the mate-rescue tests share (tests/test_rescue_cpu.py, tests/test_gpu_rescue.py): named, deterministic cases of a few
transcripts of at most about 3 kb with hand-made orphan records -- the smallest shapes at which the rule (csrc/rescuefmt.h) or the
kernel (csrc/rescue.hip) can go wrong -- each with the (permille, window) pairs it is run at; a few hundred random small jobs; and
the end-to-end batch: a spliced synthetic transcriptome whose reads the restated scan contract (oracle.mapper_oracle.scan_reads)
maps.  Built once a process."""
import functools
import struct

import numpy as np

from oracle import mapper_oracle as MO
from oracle import oracle as O

COMP = bytes.maketrans(b"ACGTacgtN", b"TGCAtgcaN")
ACGT = np.frombuffer(b"ACGT", np.uint8)
# the kernel's bounds (csrc/rescuefmt.h): candidates a round, candidates a staged tile, bases of a mate the packed form holds
LANES, TILE, MATE_MAX = 64, 1024, 512
STATS = ("reads_eligible", "records_orphan", "jobs_with_candidates", "candidates", "reads_rescued", "records_rescued", "records_dropped", "sum_mism")


def revcomp(s):
    return s.translate(COMP)[::-1]


def rand(rng, n):
    return bytes(rng.choice(ACGT, n))


def sub(read, *at):
    """the read with the bases at `at` replaced by another base"""
    b = bytearray(read)
    for i in at:
        b[i] = {65: 67, 67: 71, 71: 84, 84: 65, 97: 99, 99: 103, 103: 116, 116: 97}[b[i]]
    return bytes(b)


def on_strand(bases, fwd):
    """the read whose oriented bases on strand `fwd` are `bases`"""
    return bases if fwd else revcomp(bases)


class Batch:
    """reads with hand-made records, in order"""

    def __init__(self, seqs):
        self.seqs, self.r1, self.r2, self.recs, self.off = list(seqs), [], [], [], [0]

    def read(self, m1, m2, recs):
        self.r1.append(m1); self.r2.append(m2); self.recs.extend(recs); self.off.append(len(self.recs))

    def orphan(self, tid, st, f, p, la, x, lb, subs=(), others=()):
        """a read with one orphan record (and `others`): the anchor -- mate 1 for st 1, mate 2 for st 2 -- copied from transcript tid
        at p (la bases, strand f), the missing mate from x (lb bases, strand 1 - f) with substitutions at `subs`"""
        t = self.seqs[tid]
        anchor = on_strand(t[max(p, 0):max(p, 0) + la].ljust(la, b"A")[:la], f)
        mate = on_strand(sub(t[x:x + lb], *subs), 1 - f)
        rec = (tid, p, 0, 0, la & 0xFFFF, lb & 0xFFFF, f, 0, st, 0)
        self.read(*((anchor, mate) if st == 1 else (mate, anchor)), [rec, *others])

    def case(self, *opts):
        return dict(seqs=self.seqs, r1=self.r1, r2=self.r2, hits=np.array(self.recs, dtype=O.HIT_DTYPE) if self.recs else np.zeros(0, O.HIT_DTYPE),
                    off=np.asarray(self.off, np.uint32), opts=list(opts))


def _strands(rng):
    b = Batch([rand(rng, 600)])
    for st in (1, 2):
        b.orphan(0, st, 1, 100, 40, 330, 50, subs=(7,))              # anchor forward: the mate lies downstream
        b.orphan(0, st, 0, 400, 40, 150, 50, subs=(7,))              # anchor reverse: upstream
    return b.case((900, 400), (1000, 400))


def _clipping(rng):
    t = rand(rng, 500)
    b = Batch([t])
    b.orphan(0, 1, 0, 30, 40, 0, 50)                                 # the window runs off the start: x = 0 is the first candidate
    b.orphan(0, 2, 1, 380, 40, 450, 50)                              # ... off the end: x = tlen - lb the last
    b.orphan(0, 1, 1, 100, 40, 100, 50)                              # x == p: in
    b.orphan(0, 1, 1, 100, 40, 99, 50)                               # x == p - 1: out
    b.orphan(0, 2, 0, 300, 40, 290, 50)                              # x + lb == p + la: in
    b.orphan(0, 2, 0, 300, 40, 291, 50)                              # one more: out
    b.orphan(0, 1, 1, 100, 40, 250, 50)                              # x + lb == p + W at W = 200 (in), out at W = 199
    b.orphan(0, 2, 0, 300, 40, 140, 50)                              # x == p + la - W at W = 200 (in), out at W = 199
    b.orphan(0, 1, 1, 100, 40, 100, 50)                              # W = 49 < lb: no candidates
    b.orphan(0, 1, 1, -5, 40, 0, 50)                                 # the anchor at a negative pos
    b.orphan(0, 2, 0, 480, 40, 450, 50)                              # the anchor hangs over the end
    b.orphan(0, 1, 1, -300, 40, 0, 50)                               # the whole window in front of the transcript
    b.orphan(0, 2, 0, 900, 40, 450, 50)                              # ... and the anchor far behind it
    return b.case((1000, 200), (1000, 199), (1000, 49), (1000, 50), (1000, 1 << 20))


def _sizes(rng):
    t = rand(rng, 300)
    b = Batch([t, t[50:110], b"ACGTACGTAC"])
    b.orphan(1, 1, 1, 0, 20, 0, 60, subs=(3,))                       # lb == tlen
    b.read(on_strand(t[50:70], 1), on_strand(t[50:111], 0), [(1, 0, 0, 0, 20, 61, 1, 0, 1, 0)])      # lb == tlen + 1
    b.read(on_strand(t[50:70], 1), b"", [(0, 50, 0, 0, 20, 0, 1, 0, 1, 0)])                           # lb == 0
    b.read(b"", on_strand(t[60:90], 1), [(0, 10, 0, 0, 30, 0, 0, 0, 2, 0)])                           # ... of mate 1, the anchor mate 2 reverse
    b.read(b"", on_strand(t[100:130], 0), [(0, 50, 0, 0, 0, 30, 1, 0, 1, 0)])                         # la == 0: the window begins at p
    b.orphan(2, 2, 0, 0, 10, 0, 10)                                  # a transcript shorter than one 16-byte load
    b.orphan(2, 1, 1, 0, 4, 3, 7, subs=(6,))
    return b.case((900, 1000), (0, 1000), (800, 5))


def _budget(rng):
    b = Batch([rand(rng, 500)])
    for k in (0, 1, 4, 5, 6, 10):                                    # lb = 50 at 900: the budget is 5
        b.orphan(0, 1, 1, 60, 40, 200, 50, subs=range(2, 2 + 4 * k, 4))
        b.orphan(0, 2, 0, 300, 40, 120, 50, subs=range(1, 1 + 3 * k, 3))
    for k in (1, 2):                                                 # lb = 19 at 900: 1.9 -> 1
        b.orphan(0, 1, 1, 60, 40, 222, 19, subs=range(k))
    return b.case((900, 300), (1000, 300), (0, 300), (880, 300), (881, 300))


def _letters(rng):
    t = bytearray(rand(rng, 400))
    t[215], t[230] = ord("N"), ord("n")
    t = bytes(t)
    b = Batch([t, t.lower()])
    n_mate = bytearray(t[200:250]); n_mate[5] = ord("N")
    b.read(t[100:140], revcomp(bytes(n_mate)), [(0, 100, 0, 0, 40, 50, 1, 0, 1, 0)])                  # N in the mate, N / n in the transcript, N against N
    b.orphan(0, 1, 1, 100, 40, 200, 50)                              # (t[215] = N copied into the mate: N against N is a mismatch)
    b.orphan(1, 2, 0, 300, 40, 150, 50, subs=(9,))                   # a lower-case transcript
    b.read(t[100:140].lower(), revcomp(t[260:310]).lower(), [(0, 100, 0, 0, 40, 50, 1, 0, 1, 0)])     # lower-case mates
    b.read(t[100:140], b"*" * 50, [(0, 100, 0, 0, 40, 50, 1, 0, 1, 0)])                               # no base at all
    return b.case((900, 300), (960, 300), (940, 300), (0, 300))


def _ties(rng):
    seg, seg2 = rand(rng, 40), rand(rng, 40)
    t0 = rand(rng, 100) + seg + rand(rng, 77) + seg + rand(rng, 100)                                  # two exact copies: 100 and 217
    t1 = rand(rng, 100) + sub(seg2, 3, 30) + rand(rng, 61) + seg2 + rand(rng, 150)                    # a worse one first: 100, then 201
    t2 = b"A" * 300
    t3 = rand(rng, 30) + seg + rand(rng, TILE + 100) + seg + rand(rng, 80)                            # equal copies in two tiles: 30 and 1194
    b = Batch([t0, t1, t2, t3])
    b.read(t0[20:60], revcomp(seg), [(0, 20, 0, 0, 40, 40, 1, 0, 1, 0)])
    b.read(revcomp(seg), t0[20:60], [(0, 20, 0, 0, 40, 40, 1, 0, 2, 0)])                              # the same as status 2: mate 1 is searched
    b.read(t1[20:60], revcomp(seg2), [(1, 20, 0, 0, 40, 40, 1, 0, 1, 0)])
    b.read(revcomp(t1[300:340]), seg2, [(1, 300, 0, 0, 40, 40, 0, 0, 1, 0)])                          # from the other side: the window ends at the anchor
    b.read(b"A" * 30, b"T" * 30, [(2, 10, 0, 0, 30, 30, 1, 0, 1, 0)])                                 # a homopolymer: every candidate ties
    b.read(b"T" * 30, b"A" * 30, [(2, 250, 0, 0, 30, 30, 0, 0, 1, 0)])
    b.read(b"A" * 30, b"T" * 29 + b"G", [(2, 10, 0, 0, 30, 30, 1, 0, 1, 0)])                          # ... with one mismatch each
    b.read(t3[0:30], revcomp(seg), [(3, 0, 0, 0, 30, 40, 1, 0, 1, 0)])
    return b.case((900, 2000), (1000, 2000), (0, 2000), (900, 250))


def _lanes(rng):
    """windows of 63 / 64 / 65 candidates and of one below, at and above a tile and two tiles, the only passing candidate the LAST one
    (a round or a tile cut short loses it), and at permille 0 the first of the best"""
    t = rand(rng, 2 * TILE + 400)
    b = Batch([t])
    windows = []
    for n in (LANES - 1, LANES, LANES + 1, 2 * LANES, TILE - 1, TILE, TILE + 1, TILE + LANES, 2 * TILE, 2 * TILE + 1):
        lb = 50
        b.orphan(0, 1, 1, 100, 40, 100 + n - 1, lb, subs=(0, 49))    # forward anchor: candidates 100 .. 100 + n - 1 at W = n - 1 + lb
        b.orphan(0, 2, 0, 2 * TILE + 300, 40, 2 * TILE + 340 - (n - 1) - lb, lb, subs=(1,))      # reverse anchor: the lowest candidate
        windows.append(n - 1 + lb)
    return b.case(*[(950, w) for w in windows], (0, windows[-1]))


def _mates(rng):
    """mates one below, at and above what the packed form holds, longer ones, and window = 2^20"""
    t = rand(rng, 3000)
    b = Batch([t, rand(rng, 700)])
    for lb in (MATE_MAX - 1, MATE_MAX, MATE_MAX + 1, MATE_MAX + 16, 1200):
        b.orphan(0, 1, 1, 50, 60, 700, lb, subs=range(5, lb, 97))
        b.orphan(0, 2, 0, 2900, 60, 1500, lb, subs=range(0, lb, 61))
    for lb in (15, 16, 17, 31, 32, 33, 255, 256, 257):
        b.orphan(1, 1, 1, 20, 30, 300, lb, subs=(lb // 2,))
    return b.case((900, 2500), (990, 1 << 20), (0, 1700))


def _reads(rng):
    """what a read's records become: several orphans of which only some are placed; left and right orphans on one transcript and
    strand; equal keys; and reads that are not eligible -- status 3, status 0, a mix, no records -- between eligible ones"""
    s1, s2 = rand(rng, 40), rand(rng, 40)
    t0 = rand(rng, 100) + s1 + rand(rng, 60) + s2 + rand(rng, 60) + revcomp(s1) + rand(rng, 60) + revcomp(s2) + rand(rng, 100)
    a1, a2, r1s, r2s = 100, 200, 300, 400                           # s1, s2, revcomp(s1), revcomp(s2) begin here
    t1, t2 = t0[:350] + rand(rng, 80), rand(rng, 450)
    b = Batch([t0, t1, t2])
    left = lambda tid, p, f=1: (tid, p, 0, 0, 40, 40, f, 0, 1, 0)
    right = lambda tid, p, f=1: (tid, p, 0, 0, 40, 40, f, 0, 2, 0)
    b.read(s1, s2, [left(0, a1), left(1, a1), left(2, 50)])          # mate 2 reverse lies at 400 on t0 only: two orphans are dropped
    b.read(b"", b"", [])
    b.read(s1, s2, [left(0, a1), right(0, a2)])                      # left and right on one transcript and strand: the right one's pair sorts first
    b.read(s1, s2, [(0, a1, r2s, 340, 40, 40, 1, 0, 3, 0), left(1, a1)])      # a pair among the records: not eligible
    b.read(s1, s2, [left(0, a1), left(0, a1 - 30), left(0, a1 + 1)])  # equal keys: input order
    b.read(s1, s2, [(0, a1, 0, 0, 40, 0, 1, 0, 0, 0)])               # status 0
    b.read(s1, s2, [right(0, r2s, 0), left(0, a1), right(1, a2), left(0, r1s, 0)])      # keys (0, 1), (0, 1), (1, 0), (0, 0) where placed
    b.read(s1, s2, [left(2, 10), right(2, 10)])                      # nothing placed: the orphans stay
    b.read(s1, s2, [left(0, a1), (0, a1, 0, 0, 40, 40, 1, 0, 0, 0)])  # an orphan beside a status 0: not eligible
    b.read(s1, s2, [left(0, a1, 7)])                                 # fwd is any nonzero byte
    return b.case((900, 500), (1000, 500), (0, 500), (900, 320))


def _random_jobs(seed, n_reads=300):
    """random small jobs: short transcripts (N and lower case among them), records anywhere, mates planted near the anchor or random"""
    rng = np.random.default_rng(seed)
    seqs = []
    for k in range(12):
        s = bytearray(rand(rng, int(rng.integers(8, 260))))
        if k % 4 == 1:
            s[int(rng.integers(0, len(s)))] = ord("N")
        seqs.append(bytes(s).lower() if k % 5 == 2 else bytes(s))
    seqs.append(b"AC" * 90)                                          # repeats: ties
    b = Batch(seqs)
    for _ in range(n_reads):
        recs, m = [], [rand(rng, int(rng.integers(0, 70))), rand(rng, int(rng.integers(0, 70)))]
        kind = rng.random()
        for _ in range(int(rng.integers(0, 4))):
            tid = int(rng.integers(0, len(seqs))); t = seqs[tid].upper()
            st = int(rng.integers(1, 3)) if kind < 0.85 else int(rng.integers(0, 4))
            f = int(rng.integers(0, 2)); p = int(rng.integers(-20, len(t) + 10))
            miss = 2 - st if st in (1, 2) else 1                     # index of the missing mate
            if st in (1, 2) and rng.random() < 0.7 and len(t) > 12:  # plant the missing mate somewhere on the transcript, with errors
                lb = int(rng.integers(1, min(len(t), 69) + 1)); x = int(rng.integers(0, len(t) - lb + 1))
                seg = bytearray(t[x:x + lb])
                for i in np.nonzero(rng.random(lb) < 0.06)[0]:
                    seg[i] = ord("ACGT"[int(rng.integers(0, 4))])
                m[miss] = on_strand(bytes(seg), 1 - f)
            recs.append((tid, p, 0, 0, len(m[1 - miss]), len(m[miss]), f, 0, st, 0))
        b.read(m[0], m[1], recs)
    return b.case((900, 100), (0, 40), (1000, 300), (700, 1 << 20), (850, 1))


def spliced_transcriptome(rng, genes=10, isoforms=4, exons=8):
    """ten genes of four isoforms each, an isoform a subset of its gene's eight exons of 150 .. 400 bases"""
    seqs = []
    for _ in range(genes):
        ex = [rand(rng, int(rng.integers(150, 401))) for _ in range(exons)]
        for _ in range(isoforms):
            keep = rng.random(exons) < 0.7
            keep[int(rng.integers(0, exons))] = True
            seqs.append(b"".join(e for e, k in zip(ex, keep) if k))
    return seqs


def with_errors(rng, reads, rate):
    out = []
    for r in reads:
        b = bytearray(r)
        for i in np.nonzero(rng.random(len(b)) < rate)[0]:
            b[i] = {65: b"CGT", 67: b"AGT", 71: b"ACT", 84: b"ACG"}[b[i]][int(rng.integers(0, 3))]
        out.append(bytes(b))
    return out


def fragments(rng, seqs, n, read_len, frag_mean=250, frag_sd=25):
    """n inward-facing pairs of read_len bases from fragments of about frag_mean bases, either strand -> (mate 1, mate 2, transcript)"""
    r1, r2, src = [], [], []
    while len(r1) < n:
        tid = int(rng.integers(0, len(seqs))); s = seqs[tid]
        frag = max(read_len, int(round(rng.normal(frag_mean, frag_sd))))
        if frag > len(s):
            continue
        p = int(rng.integers(0, len(s) - frag + 1))
        a, b = s[p:p + read_len], revcomp(s[p + frag - read_len:p + frag])
        if rng.random() < 0.5:
            a, b = b, a
        r1.append(a); r2.append(b); src.append(tid)
    return r1, r2, src


@functools.lru_cache(maxsize=None)
def end_to_end(read_len=50, rate=0.02, n=400, seed=7):
    """the end-to-end data: names, transcripts, the pairs, their source transcripts"""
    rng = np.random.default_rng(seed)
    seqs = spliced_transcriptome(rng)
    r1, r2, src = fragments(rng, seqs, n, read_len)
    r1, r2 = with_errors(rng, r1, rate), with_errors(rng, r2, rate)
    return ["tx%d" % i for i in range(len(seqs))], seqs, r1, r2, src


E2E_OPTS = (900, 1000)


@functools.lru_cache(maxsize=None)
def _end_to_end_case():
    names, seqs, r1, r2, src = end_to_end()
    hits, off = MO.scan_reads(MO.build_scan_index(seqs), r1, r2, s=19)
    return dict(seqs=seqs, r1=r1, r2=r2, hits=np.ascontiguousarray(hits, dtype=O.HIT_DTYPE), off=np.asarray(off, np.uint32), opts=[E2E_OPTS])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case (seqs, r1, r2, hits, off, opts: the (permille, window) pairs it is run at)"""
    rng = np.random.default_rng(2024)
    out = {
        "strands": _strands(rng),
        "clipping": _clipping(rng),
        "sizes": _sizes(rng),
        "budget": _budget(rng),
        "letters": _letters(rng),
        "ties": _ties(rng),
        "lanes": _lanes(rng),
        "mates": _mates(rng),
        "reads": _reads(rng),
        "empty": Batch([rand(rng, 50)]).case((900, 1000)),
        "random_a": _random_jobs(51),
        "random_b": _random_jobs(52),
        "end_to_end": _end_to_end_case(),
    }
    return out


def runs():
    """every (case, permille, window) of the corpus"""
    return [(name, p, w) for name, c in cases().items() for p, w in c["opts"]]


def bad_tid_case():
    """`reads` with three records that name transcript M: the lowest is record 4"""
    c = dict(cases()["reads"])
    c["hits"] = c["hits"].copy()
    c["hits"]["tid"][[9, 4, 12]] = len(c["seqs"])
    return c


@functools.lru_cache(maxsize=None)
def expected(name, permille, window):
    """rescue_mates_host of a case: computed once, shared, never changed"""
    from sailfish_amd import hits as H
    c = cases()[name]
    h, o, m, st = H.rescue_mates_host(c["seqs"], c["hits"], c["off"], c["r1"], c["r2"], permille, window)
    for a in (h, o, m):
        a.setflags(write=False)
    return h, o, m, st


def packed(seqs):
    """list of bytes -> (the bytes back to back, uint64 offsets[n + 1])"""
    off = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return np.frombuffer(b"".join(seqs) + b"\0", np.uint8)[:-1].copy() if seqs else np.zeros(0, np.uint8), off


def blob(name, permille, window):
    """a case with its expected result as the byte string tests/rescue_harness.cpp's stand-alone program reads"""
    c = cases()[name]
    h, o, m, st = expected(name, permille, window)
    ts, toff = packed(c["seqs"])
    s1, o1 = packed(c["r1"])
    s2, o2 = packed(c["r2"])
    tl = np.array([len(x) for x in c["seqs"]], np.uint32)
    head = struct.pack("<11Q", len(c["seqs"]), len(ts), len(c["r1"]), len(s1), len(s2), len(c["hits"]), permille, window, 1, len(h), 0)
    stats = np.array([st[k] for k in STATS], np.uint64)
    parts = [ts, toff[:-1], tl, s1, o1, s2, o2, c["hits"], c["off"], h, o, m, stats]
    return head + b"".join(np.ascontiguousarray(p).tobytes() for p in parts)
