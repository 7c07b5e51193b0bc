"""Named, deterministic cases for csrc/mapper.hip and the statements they are judged by (test infrastructure; tests/test_mapper_cpu.py
shows on the CPU that every case holds the shape it claims, tests/test_gpu_mapper.py runs them on the device).

Three statements, none of them the kernel:
  * oracle/mapper_oracle.py, the restated contract (record for record);
  * vec_table(): the sorted (key, t, p) table built with numpy (sliding windows + lexsort), so that the two large indexes cost well
    under a second; entry for entry MO.build_scan_index on the small cases;
  * judge(): a brute-force check written from include/sfgpu.h alone: every record must be TRUE on the transcripts' bases
    (soundness), and a read cut error-free from a known place must carry that place (completeness)."""
import functools

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from oracle import mapper_oracle as MO

_ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
FOLD = np.full(256, 4, np.uint8)
for _i, _b in enumerate(b"ACGT"):
    FOLD[_b] = FOLD[_b + 32] = _i


def rc(b):
    return bytes(b).translate(_COMP)[::-1]


def rnd(rng, n):
    return bytes(rng.choice(_ACGT, int(n)))


def differ(b):
    """a base that is not b (case kept out of it)"""
    return b"CGTA"[b"ACGT".index(bytes([b]).upper())]


class Case:
    """transcripts, reads1, reads2 (or None), k, max_occ, the mode (seeds = S end seeds per strand, or seed_len = s for scan),
    `why` it exists, `truth`: [(read, mate 0 / 1, t, p, fwd)] for mates cut error-free from transcript t at p (fwd = 0: reverse
    complemented), `props`: named read indices / numbers the CPU test pins, `big`: judged by the vectorised table only"""

    def __init__(self, name, why, transcripts, reads1, reads2=None, k=31, max_occ=1000, seeds=None, seed_len=None, truth=(), props=None, big=False):
        assert (seeds is None) != (seed_len is None)
        self.name, self.why, self.transcripts, self.reads1, self.reads2 = name, why, list(transcripts), list(reads1), None if reads2 is None else list(reads2)
        self.k, self.max_occ, self.seeds, self.seed_len, self.truth, self.props, self.big = k, max_occ, seeds, seed_len, list(truth), props or {}, big
        assert self.reads2 is None or len(self.reads2) == len(self.reads1)

    @property
    def scan(self):
        return self.seed_len is not None

    @property
    def min_run(self):
        return self.seed_len if self.scan else self.k


# ---- the vectorised index statement --------------------------------------------------------------------------------------------
class VecTable:
    """the sorted (key, t, p) table as three arrays; what MO.scan_groups needs of a table"""

    def __init__(self, keys, t, p):
        self.keys, self.t, self.p = keys, t, p

    def __len__(self):
        return len(self.keys)

    def __getitem__(self, sl):
        return list(zip(self.keys[sl].tolist(), self.t[sl].tolist(), self.p[sl].tolist()))

    def prefix_range(self, lo_key, hi_key):
        return int(np.searchsorted(self.keys, np.uint64(lo_key))), int(np.searchsorted(self.keys, np.uint64(hi_key)))

    def get(self, key, max_occ):
        lo, hi = self.prefix_range(key, key + 1)
        return self[lo:min(hi, lo + max_occ)]


class VecIndex:
    """what MO.map_read needs of build_index's dict: occurrences in (t, p) order, at most max_occ kept"""

    def __init__(self, table, max_occ):
        self.table, self.max_occ = table, max_occ

    def get(self, key, default=()):
        return [(t, p) for _, t, p in self.table.get(key, self.max_occ)] or default


def vec_table(transcripts, k):
    shifts = (2 * np.arange(k - 1, -1, -1)).astype(np.uint64)
    keys, ts, ps = [], [], []
    for t, s in enumerate(transcripts):
        if len(s) < k:
            continue
        win = sliding_window_view(FOLD[np.frombuffer(s, np.uint8)], k)
        ok = np.nonzero(~(win > 3).any(axis=1))[0]
        keys.append((win[ok].astype(np.uint64) << shifts).sum(axis=1, dtype=np.uint64))
        ts.append(np.full(len(ok), t, np.int64)); ps.append(ok.astype(np.int64))
    if not keys:
        return VecTable(np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros(0, np.int64))
    key, t, p = np.concatenate(keys), np.concatenate(ts), np.concatenate(ps)
    o = np.lexsort((p, t, key))
    return VecTable(key[o], t[o], p[o])


def n_positions(case):
    return sum(max(len(s) - case.k + 1, 0) for s in case.transcripts)


@functools.lru_cache(maxsize=None)
def table(name):
    c = case(name)
    return vec_table(c.transcripts, c.k)


class _Codes:
    """the transcripts' code arrays, made when asked for (32 771 transcripts, four of which are ever looked at)"""

    def __init__(self, transcripts):
        self.tr, self.memo = transcripts, {}

    def __getitem__(self, t):
        if t not in self.memo:
            self.memo[t] = FOLD[np.frombuffer(self.tr[t], np.uint8)]
        return self.memo[t]


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's (hits, offsets) for the case: paired when it has reads2 -- computed once, shared by the tests, never changed"""
    return expected_for(name, True)


@functools.lru_cache(maxsize=None)
def expected_for(name, paired):
    c = case(name)
    r2 = c.reads2 if paired else None
    if c.scan:
        si = (table(name), _Codes(c.transcripts), c.k) if c.big else MO.build_scan_index(c.transcripts, c.k)
        h, o = MO.scan_reads(si, c.reads1, r2, s=c.seed_len, max_occ=c.max_occ)
    else:
        idx = VecIndex(table(name), c.max_occ) if c.big else MO.build_index(c.transcripts, c.k, c.max_occ)
        h, o = MO.map_reads(idx, c.reads1, r2, k=c.k, seeds=c.seeds)
    h.setflags(write=False); o.setflags(write=False)
    return h, o


def scan_groups(name, read, max_groups=MO.MAX_GROUPS):
    c = case(name)
    si = (table(name), _Codes(c.transcripts), c.k) if c.big else MO.build_scan_index(c.transcripts, c.k)
    return MO.scan_groups(si, read, c.seed_len, c.max_occ, max_groups)


# ---- the brute-force judge (from the header's contract, not from the kernel or the oracle) ----------------------------------------
def _oriented(read, fwd):
    c = FOLD[np.frombuffer(bytes(read), np.uint8)]
    if fwd:
        return c
    r = c[::-1]
    return np.where(r > 3, 4, 3 - r).astype(np.uint8)


def _longest_run(q, tc, pos):
    """the longest run of positions where mate q, laid on the transcript at diagonal pos, shows the same A/C/G/T"""
    j0, j1 = max(0, -pos), min(len(q), len(tc) - pos)
    if j1 <= j0:
        return 0
    m = (q[j0:j1] == tc[pos + j0:pos + j1]) & (q[j0:j1] < 4)
    edges = np.flatnonzero(np.diff(np.concatenate(([0], m.view(np.int8), [0]))))
    return int((edges[1::2] - edges[::2]).max()) if len(edges) else 0


def _find_all(text, word):
    out, a = [], text.find(word)
    while a >= 0:
        out.append(a); a = text.find(word, a + 1)
    return out


def mate_hits(hits, off, r, paired):
    """read r's records -> (the left mate's set of (t, fwd, pos), the right mate's)"""
    left, right = set(), set()
    for h in hits[off[r]:off[r + 1]]:
        st = int(h["mate_status"])
        if st in (0, 1, 3):
            left.add((int(h["tid"]), int(h["fwd"]), int(h["pos"])))
        if st == 2:
            right.add((int(h["tid"]), int(h["fwd"]), int(h["pos"])))
        if st == 3:
            right.add((int(h["tid"]), int(h["mate_fwd"]), int(h["mate_pos"])))
    return left, right


def judge(c, hits, off, paired):
    """assert that the records (hits, off) of case c are sound, well formed and complete; -> how many completeness checks applied"""
    r2 = c.reads2 if paired else None
    tcodes = _Codes(c.transcripts)
    need = c.min_run
    assert len(off) == len(c.reads1) + 1 and off[0] == 0 and off[-1] == len(hits) and (np.diff(off.astype(np.int64)) >= 0).all()
    for r, m1 in enumerate(c.reads1):
        recs = hits[off[r]:off[r + 1]]
        m2 = None if r2 is None else r2[r]
        if len(m1) > 65535 or (m2 is not None and len(m2) > 65535):
            assert len(recs) == 0, (c.name, r, "a mate over 65 535 bases: no records")
            continue
        st = [int(x) for x in recs["mate_status"]]
        if r2 is None:
            assert all(x == 0 for x in st)
        else:
            assert all(x == 3 for x in st) or st == sorted(st) and all(x in (1, 2) for x in st), (c.name, r, st)
        for h in recs:
            t, s = int(h["tid"]), int(h["mate_status"])
            assert t < len(c.transcripts) and h["pad_"] == 0
            mine, other = (m2, m1) if s == 2 else (m1, m2)
            assert h["read_len"] == len(mine) and h["mate_len"] == (0 if other is None else len(other)), (c.name, r)
            run = _longest_run(_oriented(mine, int(h["fwd"])), tcodes[t], int(h["pos"]))
            assert run >= need, (c.name, r, "record not on the bases", t, int(h["fwd"]), int(h["pos"]), run, need)
            if s == 3:
                assert h["fwd"] != h["mate_fwd"]
                run = _longest_run(_oriented(m2, int(h["mate_fwd"])), tcodes[t], int(h["mate_pos"]))
                assert run >= need, (c.name, r, "mate not on the bases", t, run, need)
                p, p2 = int(h["pos"]), int(h["mate_pos"])
                assert h["frag_len"] == max(p + len(m1), p2 + len(m2)) - min(p, p2), (c.name, r)
            else:
                assert h["mate_pos"] == 0 and h["frag_len"] == 0 and h["mate_fwd"] == 0
        keys = [(int(h["mate_status"]) == 2, int(h["tid"]), int(h["fwd"])) for h in recs]
        assert keys == sorted(keys), (c.name, r, "records out of (transcript, strand) order")
    # completeness: which truth entries the contract promises a hit for ...
    upper = None
    promised = {}
    for r, mate, t, p, fwd in c.truth:
        m = (c.reads1, c.reads2)[mate][r]
        if mate == 1 and r2 is None:
            continue
        if len(c.reads1[r]) > 65535 or (r2 is not None and len(r2[r]) > 65535):
            continue
        q = _oriented(m, fwd)
        assert np.array_equal(q, tcodes[t][p:p + len(q)]) and (q < 4).all(), (c.name, r, "the truth entry is not an error-free cut")
        if len(q) < (need if c.scan else c.k):
            continue
        if upper is None:
            upper = [(i, bytes(s).upper()) for i, s in enumerate(c.transcripts) if len(s) >= need]
        word = _ACGT[q[:need]].tobytes()
        occ = [(i, a) for i, s in upper for a in _find_all(s, word)]
        if c.scan:                                        # seeds are prefix ranges of WHOLE k-mers
            def starts_kmer(i, a):
                w = tcodes[i][a:a + c.k]
                return len(w) == c.k and bool((w < 4).all())
            occ = [x for x in occ if starts_kmer(*x)]
            if (t, p) not in occ:
                continue
        if len(occ) > c.max_occ:
            continue
        promised[(r, mate)] = (t, fwd, min(a for i, a in occ if i == t))
    # ... and whether the records keep it: a read with paired records keeps only the transcripts on which both mates lie, so a
    # mate's hit must show there only if the other mate is promised the same transcript on the other strand
    for (r, mate), (t, fwd, first) in promised.items():
        left, right = mate_hits(hits, off, r, r2 is not None)
        if r2 is not None and (hits[off[r]:off[r + 1]]["mate_status"] == 3).any():
            other = promised.get((r, 1 - mate))
            if other is None or other[0] != t or other[1] == fwd:
                continue
        got = (left, right)[mate]
        if not c.scan and c.seeds == 2:
            assert (t, fwd, first) in got, (c.name, r, mate, "missing", (t, fwd, first), sorted(got))
        else:
            assert (t, fwd) in {(a, b) for a, b, _ in got}, (c.name, r, mate, "missing", (t, fwd), sorted(got))
    return len(promised)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def _cut(rng, seqs, n, fwd=None, t=None):
    """a read of n bases cut error-free from an ACGT-only stretch of some transcript -> (read, t, p, fwd)"""
    for _ in range(1000):
        tt = int(rng.integers(0, len(seqs))) if t is None else t
        s = seqs[tt]
        if len(s) < n:
            continue
        p = int(rng.integers(0, len(s) - n + 1))
        w = s[p:p + n]
        if (FOLD[np.frombuffer(w, np.uint8)] > 3).any():
            continue
        f = int(rng.integers(0, 2)) if fwd is None else fwd
        return (w if f else rc(w)), tt, p, f
    raise AssertionError("no clean cut")


def _small_transcriptome(rng, k):
    """about 3 000 bases: isoform-like transcripts over a shared base (k-mers occur in several), N, lower case, one shorter than k"""
    base = rnd(rng, 1400)
    seqs = []
    for t in range(6):
        a = int(rng.integers(0, 800)); s = bytearray(base[a:a + 500])
        if t == 1:
            s[200] = s[310] = ord("N")
        if t == 2:
            s = bytearray(bytes(s).lower())
        if t == 4:
            s[100:160] = bytes(s[100:160]).lower()
        seqs.append(bytes(s))
    seqs.insert(3, base[:k - 1])
    return seqs


def _mode_case(name, k, seeds=None, seed_len=None):
    rng = np.random.default_rng(1000 * k + 10 * (seeds or 0) + (seed_len or 0))
    seqs = _small_transcriptome(rng, k)
    S = seeds or 2
    r1, r2, truth = [], [], []
    for n in (0, 1, k - 1, k, k + 1, k + S - 2, k + S - 1):   # the length edges (an S-seed read of k + S - 2 bases repeats an offset)
        for fwd in (1, 0):
            if n == 0:
                r1.append(b""); r2.append(b"")
                continue
            w, t, p, f = _cut(rng, seqs, n, fwd)
            truth.append((len(r1), 0, t, p, f)); r1.append(w)
            w, t, p, f = _cut(rng, seqs, n, 1 - fwd, t)
            truth.append((len(r2), 1, t, p, f)); r2.append(w)
    for _ in range(40):
        n = int(rng.integers(k, 3 * k + 10))
        w, t, p, f = _cut(rng, seqs, n)
        truth.append((len(r1), 0, t, p, f)); r1.append(w)
        if rng.random() < 0.7:
            w2, t2, p2, f2 = _cut(rng, seqs, int(rng.integers(k, 3 * k + 10)), 1 - f, t)
            truth.append((len(r2), 1, t2, p2, f2)); r2.append(w2)
        else:
            r2.append(rnd(rng, n))
    for _ in range(6):                                      # reads with a substitution, reads with N, noise
        w, t, p, f = _cut(rng, seqs, 3 * k)
        b = bytearray(w); j = int(rng.integers(0, len(b))); b[j] = differ(b[j]); r1.append(bytes(b))
        b = bytearray(w); b[int(rng.integers(0, len(b)))] = ord("N"); r2.append(bytes(b))
    r1.append(rnd(rng, 2 * k)); r2.append(rnd(rng, k))
    why = f"k = {k}: key mask, bucket shift 2k - bits, " + (f"scan seeds of {seed_len}" if seeds is None else f"{seeds} end seeds") + "; read lengths 0, 1, k - 1 .. k + S - 1"
    return Case(name, why, seqs, r1, r2, k=k, max_occ=1000, seeds=seeds, seed_len=seed_len, truth=truth)


KS = (8, 9, 16, 19, 20, 31)
MODE_CASES = {}
for _k in KS:
    for _S in (2, 3, 8):
        MODE_CASES[f"k{_k}_S{_S}"] = functools.partial(_mode_case, k=_k, seeds=_S)
    for _s in sorted({8, min(19, _k), _k}):
        MODE_CASES[f"k{_k}_s{_s}"] = functools.partial(_mode_case, k=_k, seed_len=_s)


def _both_modes(builders, name, fn):
    """register fn(name, "end" / "scan") as name_end (two end seeds) and name_scan (the builder says how long its scan seeds are)"""
    builders[name + "_end"] = lambda n=name: fn(n + "_end", "end")
    builders[name + "_scan"] = lambda n=name: fn(n + "_scan", "scan")


def _mode(mode, scan_seed_len):
    return dict(seed_len=scan_seed_len) if mode == "scan" else dict(seeds=2)


def _reads_from(rng, seqs, k, count, lens=None):
    r1, truth = [], []
    for _ in range(count):
        n = int(rng.integers(k, 2 * k + 5)) if lens is None else lens
        w, t, p, f = _cut(rng, seqs, n)
        truth.append((len(r1), 0, t, p, f)); r1.append(w)
    return r1, truth


def _tiny_k8(name, mode):
    rng = np.random.default_rng(8)
    seqs = [rnd(rng, 100), rnd(rng, 90)]
    r1, truth = _reads_from(rng, seqs, 8, 20)
    mode = _mode(mode, 8)
    return Case(name, "k = 8 on a tiny input: 256 buckets, shift 8", seqs, r1 + [b"ACGTACG", rnd(rng, 30)], k=8, truth=truth, **mode)


def _shift0(name, mode):
    rng = np.random.default_rng(80)
    seqs = [rnd(rng, 9000) for _ in range(30)]
    r1, truth = _reads_from(rng, seqs, 8, 30, lens=30)
    r1 += [rnd(rng, 30), rnd(rng, 8), rnd(rng, 7)]
    mode = _mode(mode, 8)
    return Case(name, "k = 8 with more than 262 144 valid 8-mers: bits == 2k = 16, bucket shift 0 (scan: sh = 0 too)", seqs, r1, k=8, max_occ=64,
                truth=truth, big=True, **mode)


def _span(name):
    rng = np.random.default_rng(20)
    seqs = [rnd(rng, 66500) for _ in range(8)]
    r1, truth = _reads_from(rng, seqs, 20, 30, lens=50)
    sub = []
    for w in r1[:10]:                                       # a substitution at base 25: the 8-base windows before it still seed
        b = bytearray(w); b[25] = differ(b[25]); sub.append(bytes(b))
    return Case(name, "k = 20, more than 524 288 valid k-mers (bits = 17) and scan seeds of 8 bases (16 bits): a prefix range spans two buckets",
                seqs, r1 + sub + [rnd(rng, 50)], k=20, max_occ=64, seed_len=8, truth=truth, big=True)


M_MANY = 32771
MANY_BEARING = (0, 5, 32767, 32768, M_MANY - 1)


def _many(name, mode):
    rng = np.random.default_rng(327)
    k = 16
    seqs = [b"ACGTACGTAC"[:1 + t % 10] for t in range(M_MANY)]        # shorter than k: equal kmer_off values in long runs
    for t in MANY_BEARING:
        seqs[t] = rnd(rng, 60 + t % 7)
    r1, truth = [], []
    for t in MANY_BEARING:
        for fwd in (1, 0):
            w, tt, p, f = _cut(rng, seqs, 30, fwd, t)
            truth.append((len(r1), 0, tt, p, f)); r1.append(w)
    mode = _mode(mode, 12)
    return Case(name, "M = 32 771 > 32 768: k_index_kmers folds transcripts onto blockIdx.y + blockIdx.z * gridDim.y; k_index_locate picks the LAST "
                "transcript among equal kmer_off values (runs of transcripts shorter than k)", seqs, r1 + [rnd(rng, 30)], k=k, truth=truth, big=True,
                props={"bearing": MANY_BEARING}, **mode)


STRIDE_POSITIONS = (1023, 1024, 1025, 2500)


def _stride(name, mode):
    rng = np.random.default_rng(1024)
    k = 16
    seqs = [rnd(rng, n + k - 1) for n in STRIDE_POSITIONS]
    r1, truth = [], []
    for t, n in enumerate(STRIDE_POSITIONS):
        for p in (0, 1022, 1023, 1024, n - 1):
            if p < n:
                L = min(24, len(seqs[t]) - p)
                truth.append((len(r1), 0, t, p, 1)); r1.append(seqs[t][p:p + L])
                truth.append((len(r1), 0, t, p, 0)); r1.append(rc(seqs[t][p:p + L]))
    mode = _mode(mode, 16)
    return Case(name, "transcripts with exactly 1023, 1024, 1025 and 2500 k-mer positions: the second pass of k_index_kmers' stride loop starts at "
                "position 1024; reads at positions 1023 and 1024", seqs, r1, k=k, truth=truth, **mode)


def _all_short(name, mode):
    rng = np.random.default_rng(5)
    seqs = [rnd(rng, n) for n in (15, 1, 7, 15, 3)]
    mode = _mode(mode, 8)
    return Case(name, "every transcript shorter than k: no k-mer slot at all, every read unmapped", seqs, [seqs[0], seqs[0] + seqs[3], rnd(rng, 40), b""],
                [seqs[3], rc(seqs[0]), rnd(rng, 16), b"A"], k=16, **mode)


def _all_n(name, mode):
    rng = np.random.default_rng(6)
    seqs = [b"N" * 100]
    mode = _mode(mode, 8)
    return Case(name, "an all-N transcript: k-mer slots but n_valid = 0", seqs, [b"N" * 40, rnd(rng, 40), b"A" * 40, b"n" * 16], k=16, **mode)


def _len_k(name, mode):
    rng = np.random.default_rng(7)
    k = 16
    seqs = [rnd(rng, k), rnd(rng, k - 1), rnd(rng, 50), rnd(rng, k)]
    r1 = [seqs[0], rc(seqs[0]), seqs[1], seqs[3], rc(seqs[3]), seqs[0][1:] + b"A", b"A" + seqs[0], seqs[0] + b"A"]
    truth = [(0, 0, 0, 0, 1), (1, 0, 0, 0, 0), (3, 0, 3, 0, 1), (4, 0, 3, 0, 0)]
    mode = _mode(mode, 16)
    return Case(name, "transcripts of exactly k bases (one k-mer) and k - 1 bases (none); M = 1 lies in m1_*", seqs, r1, k=k, truth=truth, **mode)


def _m1(name, mode):
    rng = np.random.default_rng(11)
    seqs = [rnd(rng, 300)]
    r1, truth = _reads_from(rng, seqs, 16, 12)
    mode = _mode(mode, 10)
    return Case(name, "M = 1: k_index_locate's search over one transcript, a (1, 1, 1) y/z grid", seqs, r1 + [rnd(rng, 30)], k=16, truth=truth, **mode)


def _all_bytes(name, mode):
    rng = np.random.default_rng(256)
    k = 16
    a, b = rnd(rng, 60), rnd(rng, 60)
    seqs = [a + bytes(range(256)) + b, rnd(rng, 80)]
    odd = bytes([0xC1, 0xC3, 0xC7, 0xD4, 0x01, 0x03, 0x07, 0x14, 0xE1, 0xE3, 0xE7, 0xF4, 0x21, 0x23, 0x27, 0x34] * 2)    # ACGT with a bit set or cleared
    seqs.append(rnd(rng, 20) + odd + rnd(rng, 20))
    r1 = [a[20:], a[30:] + bytes(range(8)), bytes(range(250, 256)) + b[:30], b[10:50], rc(b[10:50]), odd, a[40:] + b"\0" * 16, bytes(range(0x38, 0x58))]
    truth = [(0, 0, 0, 20, 1), (3, 0, 0, 60 + 256 + 10, 1), (4, 0, 0, 60 + 256 + 10, 0)]
    mode = _mode(mode, 8)
    return Case(name, "a transcript holding every byte value once between clean flanks: only ACGTacgt are bases (0xC1, 0x01, 0x21 ... are not)", seqs, r1,
                k=k, truth=truth, **mode)


def _n_one_kmer(name, mode):
    rng = np.random.default_rng(12)
    k = 16
    a, b = rnd(rng, k), rnd(rng, k)
    seqs = [a + b"N" + b, rnd(rng, 40)]
    r1 = [a, b, rc(a), rc(b), a + b"N" + b, a[1:] + b"N" + b[:-1], a + b[:1], a[-1:] + b]
    truth = [(0, 0, 0, 0, 1), (1, 0, 0, k + 1, 1), (2, 0, 0, 0, 0), (3, 0, 0, k + 1, 0)]
    mode = _mode(mode, 16)
    return Case(name, "N placed so that exactly one k-mer survives on each side of it", seqs, r1, k=k, truth=truth, props={"n_kmers": 2 + 40 - k + 1}, **mode)


# -- reads, end seeds
def _end_edges(name, S=2):
    rng = np.random.default_rng(31 + S)
    k = 16
    T = rnd(rng, 200)
    pal = rnd(rng, 12); pal = pal + rc(pal)                  # its own reverse complement, 24 bases
    U, V, J, Mid = rnd(rng, k), rnd(rng, k), rnd(rng, 9), rnd(rng, 5)
    seqs = [T, rnd(rng, 30) + pal + rnd(rng, 30), U + J + V + rnd(rng, 10)]
    w = T[50:50 + 40]
    props, r1 = {}, []

    def add(key, read):
        props[key] = len(r1); r1.append(read)
    for strand, orient in (("fwd", lambda x: x), ("rc", rc)):
        add("N_seed0_" + strand, orient(w[:3] + b"N" + w[4:]))
        add("N_seed1_" + strand, orient(w[:-4] + b"N" + w[-3:]))
        add("N_middle_" + strand, orient(w[:20] + b"N" + w[21:]))
    add("negative_pos", rnd(rng, 7) + T[:k])                # junk + transcript[0:k]: pos = -7
    add("negative_pos_rc", rc(rnd(rng, 7) + T[:k]))
    add("overhang", T[-k:] + rnd(rng, 9))                    # transcript tail + junk: the read hangs 9 bases over the end
    add("overhang_rc", rc(T[-k:] + rnd(rng, 9)))
    add("palindrome", pal)
    add("seeds_disagree", U + Mid + V)                       # seed 0 says pos 0, seed 1 says pos 4: the first one wins
    add("seeds_disagree_rc", rc(U + Mid + V))
    # a read of k + S - 2 bases (S > 2: seeds 0 and 1 share offset 0, the second is dropped): transcript 3 holds its first window
    # only, transcript 4 its last window only -- one vote each, both kept; a duplicate of seed 0 that voted would leave 3 alone
    D = rnd(rng, k + max(S, 3) - 2)
    seqs.append(rnd(rng, 12) + D[:k] + bytes([differ(D[k])]) + rnd(rng, 12))
    seqs.append(rnd(rng, 9) + bytes([differ(D[-k - 1])]) + D[-k:] + rnd(rng, 12))
    add("shared_offset", D)
    add("shared_offset_rc", rc(D))
    return Case(name, "end-seed reads: N in one seed window only, pos < 0, overhang past the end, a palindromic read, seeds that disagree", seqs, r1,
                k=k, seeds=S, props=props)


OCC = 4                                                     # the max_occ of the triple


def _maxocc_triple(name, mode):
    """three words X[0], X[1], X[2] of k bases with OCC - 1, OCC and OCC + 1 occurrences, spread over transcripts 0 .. 3 in an order in which
    (transcript, position) order differs from the order of planting; transcript 1 holds two occurrences of each"""
    rng = np.random.default_rng(44)
    k = 16
    X = [rnd(rng, k) for _ in range(3)]
    plan = {0: [3, 1, 1], 1: [0, 3, 1, 1], 2: [2, 0, 3, 1, 1]}                     # word -> the transcripts that hold it
    parts = {t: [] for t in range(4)}
    for w in (2, 0, 1):
        for t in plan[w]:
            parts[t].append(X[w])
    seqs = []
    for t in range(4):
        s = rnd(rng, 11)
        for x in parts[t]:
            s += x + rnd(rng, int(rng.integers(5, 12)))
        seqs.append(s)
    seqs.append(rnd(rng, 50))
    tails = [rnd(rng, 10) for _ in range(3)]
    r1 = [X[w] + tails[w] for w in range(3)] + [rc(X[w] + tails[w]) for w in range(3)] + list(X)
    mode = _mode(mode, 16)
    return Case(name, "words with exactly max_occ - 1, max_occ and max_occ + 1 occurrences: end seeds keep the first max_occ in (transcript, position) "
                "order, scan mode misses", seqs, r1, k=k, max_occ=OCC, props={"words": X, "counts": [OCC - 1, OCC, OCC + 1]}, **mode)


def _maxocc1(name, mode):
    rng = np.random.default_rng(45)
    k = 16
    x, y = rnd(rng, 20), rnd(rng, 20)
    seqs = [rnd(rng, 10) + x + rnd(rng, 10), rnd(rng, 5) + x + rnd(rng, 12) + y, rnd(rng, 40)]
    r1 = [x, y, rc(x), rc(y), x[2:] + seqs[0][30:34]]
    mode = _mode(mode, 16)
    return Case(name, "max_occ = 1: a word that occurs once maps, a word that occurs twice keeps its first occurrence (end seeds) or misses (scan)", seqs, r1,
                k=k, max_occ=1, truth=[(1, 0, 1, 37, 1), (3, 0, 1, 37, 0)], **mode)


# -- reads, scan
def _scan_cap(name):
    """nine 14-base segments, alternating strands, each on a transcript of its own: 5 groups on the forward walk, 4 on the reverse one,
    9 in all -- the cap of 8 is shared by the two strands"""
    rng = np.random.default_rng(89)
    k, s, seg = 12, 10, 14
    segs = [rnd(rng, seg) for _ in range(9)]
    read = b"".join(x if j % 2 == 0 else rc(x) for j, x in enumerate(segs))
    seqs = []
    for j, x in enumerate(segs):
        nxt = read[seg * (j + 1)] if j % 2 == 0 and j < 8 else (rc(read)[seg * (9 - j)] if j % 2 == 1 else ord("A"))
        seqs.append(rnd(rng, 9) + x + bytes([differ(nxt)]) + rnd(rng, 15))
    five = b"".join(x if j % 2 == 0 else rc(x) for j, x in enumerate(segs[:5]))
    return Case(name, "the scan group cap: kScanGroups = 8 shared by both strands; a ninth available group is ignored", seqs, [read, rc(read), five], k=k,
                seed_len=s, props={"nine": 0, "nine_rc": 1, "five": 2})


def _scan_edges(name):
    rng = np.random.default_rng(90)
    k, s = 16, 10
    T = rnd(rng, 200)
    U = rnd(rng, 60)
    pal = rnd(rng, 15); pal = pal + rc(pal)
    R = rnd(rng, 40)                                         # the reverse-strand read, as it lies on transcript 3
    low = bytearray(rnd(rng, 120)); low[40:70] = bytes(low[40:70]).lower()
    tn = bytearray(rnd(rng, 120)); tn[60] = ord("N")
    rcR = rc(R)
    decoy = rnd(rng, 20) + rcR[:s + 3] + bytes([differ(rcR[s + 3])]) + rnd(rng, 30)      # the forward walk's first window lands here, partially
    seqs = [T, U, rnd(rng, 25) + pal + rnd(rng, 25), rnd(rng, 30) + R + rnd(rng, 30), decoy, bytes(low), bytes(tn), rnd(rng, 80)]
    props, r1, truth = {}, [], []

    def add(key, read, tr=None):
        props[key] = len(r1)
        if tr is not None:
            truth.append((len(r1), 0) + tr)
        r1.append(read)
    add("whole_fwd", T[30:90], (0, 30, 1))
    add("whole_rev_after_fwd_partial", rcR, (3, 30, 0))
    add("palindrome", pal, (2, 25, 1))
    add("tail_only", T[-(k - 1):])                           # lies wholly inside the last k - 1 bases: no k-mer starts there
    add("tail_only_rc", rc(T[-(k - 1):]))
    add("stop_read_end", T[100:100 + 25], (0, 100, 1))
    add("stop_transcript_end", U[-30:] + rnd(rng, 12), None)
    add("stop_read_N", T[40:65] + b"N" + T[66:80])
    add("stop_transcript_N", bytes(tn[30:60]) + b"A" + bytes(tn[61:90]))
    add("lower_case_run", bytes(low[20:100]).upper(), (5, 20, 1))
    add("lower_case_read", bytes(low[20:100]).lower(), (5, 20, 1))
    b = bytearray(T[10:100])
    for j in range(s - 1, len(b), s):
        b[j] = ord("N")
    add("N_every_s_minus_1", bytes(b))                       # runs of s - 1 clean bases: no window
    b = bytearray(T[10:100]); keep = bytes(b[-s:])
    for j in range(s - 1, len(b) - s, s):
        b[j] = ord("N")
    b[len(b) - s - 1] = ord("N"); b[-s:] = keep
    add("one_window_at_the_end", bytes(b))
    add("one_window_at_the_end_rc", rc(bytes(b)))
    add("shorter_than_s", T[5:5 + s - 1])
    add("exactly_s", T[5:5 + s], (0, 5, 1))
    return Case(name, "scan reads: whole-read matches on either strand, a palindrome, the transcript's last k - 1 bases, what stops an extension, "
                "reads whose N leave no window or one", seqs, r1, k=k, seed_len=s, truth=truth, props=props)


# -- pairs
def _pairs(name, mode):
    rng = np.random.default_rng(60)
    k = 16
    X, Y = rnd(rng, 30), rnd(rng, 30)
    A = rnd(rng, 20) + X + rnd(rng, 25) + rc(Y) + rnd(rng, 22) + Y + rnd(rng, 18) + rc(X) + rnd(rng, 20)     # X, Y on both strands of A
    shared1, shared2 = rnd(rng, 40), rnd(rng, 40)
    B = rnd(rng, 30) + shared1 + rnd(rng, 60) + shared2 + rnd(rng, 30)
    Cc = rnd(rng, 10) + shared2 + rnd(rng, 70)
    D = rnd(rng, 12) + shared1 + rnd(rng, 50)
    E = rnd(rng, 150)
    seqs = [A, B, Cc, D, E]
    props, r1, r2 = {}, [], []

    def add(key, a, b):
        props[key] = len(r1); r1.append(a); r2.append(b)
    add("cross_product", X + rnd(rng, 20), Y + rnd(rng, 20))  # left {(A,0), (A,1)} x right {(A,0), (A,1)} -> two pairs, left-major
    add("same_strand", E[10:50], E[90:130])                  # both mates forward on E: no pair, orphans
    add("same_strand_rc", rc(E[10:50]), rc(E[90:130]))
    add("left_BD_right_BC", shared1, rc(shared2))            # left hits {B, D}, right hits {B, C}: one pair on B
    add("mate_inside", E[20:80], rc(E[35:65]))               # one mate inside the other
    add("mate_inside_swapped", rc(E[35:65]), E[20:80])
    add("negative_and_overhang", rnd(rng, 9) + E[:25], rc(E[-25:] + rnd(rng, 11)))     # pos < 0 and an end past the transcript feed frag_len
    add("negative_and_overhang_swapped", rc(E[-25:] + rnd(rng, 11)), rnd(rng, 9) + E[:25])
    add("left_only", E[30:70], rnd(rng, 40))
    add("right_only", rnd(rng, 40), rc(E[30:70]))
    add("both_unmapped", rnd(rng, 40), rnd(rng, 33))
    add("different_transcripts", E[30:70], rc(Cc[90:120]))
    add("different_lengths", E[10:27], rc(E[60:140]))
    add("empty_left", b"", rc(E[60:100]))
    add("short_right", E[60:100], b"ACGT")
    mode = _mode(mode, 12)
    return Case(name, "pairing, case by case: cross product, same-strand mates, {B, D} x {B, C}, a mate inside the other, negative positions and overhang "
                "in frag_len, orphans of either side, mates of different lengths", seqs, r1, r2, k=k, props=props, **mode)


def _capacity(name, mode):
    rng = np.random.default_rng(70)
    k = 16
    shared = rnd(rng, 60)
    seqs = [rnd(rng, 5 + t) + shared + rnd(rng, 10) for t in range(40)]
    r1 = [shared[a:a + 30] if a % 2 == 0 else rc(shared[a:a + 30]) for a in range(30)]
    mode = _mode(mode, 12)
    return Case(name, "30 reads with 40 records each: more than max(4 n, 1024) records, so QuasiIndex.map_reads has to call twice", seqs, r1, k=k, **mode)


LONG_LENS = (65535, 65536)


def _long_mate(name, mode):
    rng = np.random.default_rng(66)
    T = rnd(rng, 66000)
    short = rc(T[65900:65950])
    long_ok, long_bad = T[100:100 + 65535], T[100:100 + 65536]
    r1 = [long_ok, long_bad, short, short, rc(long_ok), rc(long_bad)]
    r2 = [short, short, long_ok, long_bad, T[65900:65950], T[65900:65950]]
    truth = [(0, 0, 0, 100, 1), (0, 1, 0, 65900, 0), (2, 0, 0, 65900, 0), (2, 1, 0, 100, 1), (3, 0, 0, 65900, 0), (4, 0, 0, 100, 0), (4, 1, 0, 65900, 1)]
    mode = _mode(mode, 16)
    return Case(name, "mates of 65 535 and 65 536 bases: at 65 535 the records carry the true lengths and fragment, above it the read gets no records", [T],
                r1, r2, k=16, truth=truth, big=True, **mode)


def _no_candidate(name, mode):
    rng = np.random.default_rng(71)
    seqs = [rnd(rng, 200)]
    mode = _mode(mode, 16)
    return Case(name, "a batch with no candidate at all: zero-length candidate and record buffers", seqs, [rnd(rng, 40) for _ in range(5)],
                [rnd(rng, 40) for _ in range(5)], k=16, **mode)


BUILDERS = dict(MODE_CASES)
for _n, _f in (("tiny_k8", _tiny_k8), ("shift0_k8", _shift0), ("many_transcripts", _many), ("stride", _stride), ("all_short", _all_short), ("all_N", _all_n),
               ("len_k", _len_k), ("m1", _m1), ("all_bytes", _all_bytes), ("n_one_kmer", _n_one_kmer), ("maxocc_triple", _maxocc_triple), ("maxocc1", _maxocc1),
               ("pairs", _pairs), ("capacity", _capacity), ("long_mate", _long_mate), ("no_candidate", _no_candidate)):
    _both_modes(BUILDERS, _n, _f)
BUILDERS["span_k20_s8"] = lambda: _span("span_k20_s8")
for _S in (2, 3, 8):
    BUILDERS[f"end_edges_S{_S}"] = functools.partial(_end_edges, f"end_edges_S{_S}", _S)
BUILDERS["scan_cap"] = lambda: _scan_cap("scan_cap")
BUILDERS["scan_edges"] = lambda: _scan_edges("scan_edges")
for _n, _f in list(MODE_CASES.items()):
    BUILDERS[_n] = functools.partial(_f, _n)

CASE_NAMES = tuple(BUILDERS)
BIG = ("shift0_k8_end", "shift0_k8_scan", "span_k20_s8", "many_transcripts_end", "many_transcripts_scan", "long_mate_end", "long_mate_scan")


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    assert c.name == name and c.big == (name in BIG), name
    return c
