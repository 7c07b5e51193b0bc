"""The shared corpus of the genome coverage tests (tests/test_covgenome_cpu.py, tests/test_gpu_covgenome.py): one exon model, built
as genes.ExonModel.for_names returns it, and one set of records whose transcript runs (hits.coverage_host) hold every edge of
csrc/covgfmt.h's rule, each on a transcript of its own so that it stays a run of its own.  Four chromosomes, numbered in the bytewise
order of their names: chr1, chr2, chr9xxx... (5 000 bytes) and chrE, which no transcript touches (an empty run list).

  inside / at_end / at_start   chr1 +, blocks of 50, 30 and 40 bases: a run inside block 0, one that ends exactly at block 0's end,
                               one (of another sum) that starts exactly at block 1's start
  plus3, minus3                a run over three blocks of 10 bases, on + and the same on -
  edge_hi, single              the base 4 294 967 294 of chr1 (the last a block may hold) and base 0 of chr2 at equal sums: two rows
  onebase                      three 1-base exons under one run
  wave300                      ONE run over 300 one-base blocks on -: the wavefront path
  thresh                       runs of exactly 8 and 9 pieces: either side of the threshold between the two emit kernels
  iso_a, iso_b                 two isoforms sharing their first exon: the sums add
  touch_eq_a / _b              pieces that touch with EQUAL sums: one row
  touch_ne_a / _b              pieces that touch with unequal sums: two rows
  meet_a / _b / _c             -s and +s meet on one key with a third event: the neighbours differ by that one alone
  intron0                      two blocks of one transcript that touch
  far                          a block at 4 000 000 000: positions beyond 2^31
  longname                     the chromosome with 5 000 bytes of name
  st1 .. st4                   transcripts of every status but 0, with runs: dropped whole
  short_model                  blocks of 30 bases under a transcript of 50: a run across L and one wholly beyond it
  long_model                   blocks of 80 bases under a transcript of 50
  empty                        ref_len 0, placed, no blocks
  big_a, big_b                 one block shared; no records -- BIG_RUNS gives each a run of (2^31 - 1) 2^32 for the CPU tests, which
                               add to 2^64 - 2^33 without wrapping (on the device a sum like it would need 2^31 records)
  wave_more                    300 one-base blocks more; no records here -- the edge corpora put their long runs on it
  rand0 .. rand7               isoforms over one region of chr2, both strands, and 4 000 random records

EDGES lists the edge corpora: the named records, a prefix of the random ones and some runs of 20 pieces on wave_more, chosen (by a
search over the prefixes, its result written down here and asserted by edge_expected) so that each count a kernel's grid is sized by
falls one below, on and one above a multiple of the 256 lanes of a block: the transcript runs (k_covg_count, k_covg_emit), the
pieces (the events are two a piece, so they fall two below, on and two above: k_covg_gather, k_covg_tail_flag and _compact, where
"on" also puts the last event, whose `i + 1 == n`, in a block's last lane), the distinct keys (k_covg_open_flag, k_covg_run_write),
the genome runs (k_covg_bases); and the long runs 3, 4 and 5, around the 4 wavefronts of a block of k_covg_emit_long.
"""
import collections
import functools

import numpy as np

import coverage_corpus as cc

HIT_DTYPE = cc.HIT_DTYPE
Placement = collections.namedtuple("Placement", "status chrom strand exon_off exon_start exon_len n_chrom chrom_names")
CHROM_NAMES = [b"chr1", b"chr2", b"chr9" + b"x" * 4996, b"chrE"]
FAR = 4_000_000_000
BLOCK = 256                                                # the lanes of a block in coverage_genome.hip's kernels


def _model():
    """-> list of (name, ref_len, status, chrom, strand, blocks ascending along the genome) and the records (name, pos, len, p)"""
    rng = np.random.default_rng(39)
    T, R = [], []
    t = lambda *a: T.append(a)                             # noqa: E731
    r = lambda *a: R.append(a)                             # noqa: E731
    for name, (pos, n, p) in (("inside", (5, 10, 0.5)), ("at_end", (30, 20, 0.25)), ("at_start", (50, 10, 0.125))):
        t(name, 120, 0, 0, 1, [(100, 50), (200, 30), (300, 40)])
        r(name, pos, n, p)
    t("plus3", 30, 0, 0, 1, [(1000, 10), (1020, 10), (1040, 10)]); r("plus3", 5, 20, 0.5)
    t("minus3", 30, 0, 0, -1, [(2000, 10), (2020, 10), (2040, 10)]); r("minus3", 5, 20, 0.5)
    t("edge_hi", 1, 0, 0, 1, [(4294967294, 1)]); r("edge_hi", 0, 1, 0.5)
    t("single", 100, 0, 1, 1, [(0, 100)]); r("single", 0, 10, 0.5)
    t("onebase", 3, 0, 1, 1, [(200, 1), (202, 1), (204, 1)]); r("onebase", 0, 3, 0.75)
    t("wave300", 300, 0, 1, -1, [(1000 + 2 * i, 1) for i in range(300)]); r("wave300", 0, 300, 0.375)
    t("thresh", 20, 0, 1, 1, [(3000 + 2 * i, 1) for i in range(20)]); r("thresh", 0, 8, 0.5); r("thresh", 8, 9, 0.25)
    t("iso_a", 200, 0, 0, 1, [(5000, 100), (5200, 100)]); r("iso_a", 10, 50, 0.5); r("iso_a", 90, 30, 0.25)
    t("iso_b", 150, 0, 0, 1, [(5000, 100), (5400, 50)]); r("iso_b", 20, 60, 0.25); r("iso_b", 95, 20, 0.5)
    t("touch_eq_a", 50, 0, 0, 1, [(6000, 50)]); r("touch_eq_a", 0, 50, 0.5)
    t("touch_eq_b", 50, 0, 0, -1, [(6050, 50)]); r("touch_eq_b", 0, 50, 0.5)
    t("touch_ne_a", 50, 0, 0, 1, [(6200, 50)]); r("touch_ne_a", 0, 50, 0.5)
    t("touch_ne_b", 50, 0, 0, 1, [(6250, 50)]); r("touch_ne_b", 0, 50, 0.25)
    t("meet_a", 50, 0, 0, 1, [(6400, 50)]); r("meet_a", 0, 50, 0.5)
    t("meet_b", 50, 0, 0, 1, [(6450, 50)]); r("meet_b", 0, 50, 0.5)
    t("meet_c", 30, 0, 0, -1, [(6450, 30)]); r("meet_c", 0, 30, 0.125)
    t("intron0", 20, 0, 0, 1, [(7000, 10), (7010, 10)]); r("intron0", 5, 10, 0.5)
    t("far", 100, 0, 1, 1, [(FAR, 60), (FAR + 100, 40)]); r("far", 10, 80, 0.5)
    t("longname", 20, 0, 2, 1, [(10, 20)]); r("longname", 0, 20, 0.5)
    for s in (1, 2, 3, 4):
        t(f"st{s}", 50, s, -1, 0, []); r(f"st{s}", 10, 10 * s, 0.5)
    t("short_model", 50, 0, 0, 1, [(8000, 30)]); r("short_model", 20, 20, 0.5); r("short_model", 42, 6, 0.25)
    t("long_model", 50, 0, 0, 1, [(8100, 80)]); r("long_model", 0, 50, 0.5)
    t("empty", 0, 0, 0, 1, [])
    t("big_a", 10, 0, 0, 1, [(9000, 10)])
    t("big_b", 10, 0, 0, -1, [(9000, 10)])
    t("wave_more", 300, 0, 0, 1, [(12000 + 2 * i, 1) for i in range(300)])
    exons = [(20000 + 150 * i, int(rng.integers(20, 61))) for i in range(40)]          # the region's exons; an isoform takes some of them
    for k in range(8):
        mine = [e for e in exons if rng.random() < 0.5] or exons[:1]
        total = sum(n for _, n in mine)
        t(f"rand{k}", total + (k % 3) - 1, 0, 1, 1 if k % 2 == 0 else -1, mine)       # lengths beside, at and beyond the blocks' total
        for _ in range(500):
            n = int(rng.integers(30, 71))
            r(f"rand{k}", int(rng.integers(-10, total)), n, float(rng.integers(1, 257)) / 256)
    return T, R


# (count, random records, long runs on wave_more, the count's value): see the docstring
EDGES = (("transcript_runs", 362, 0, 511), ("transcript_runs", 1054, 0, 1280), ("transcript_runs", 363, 0, 513),
         ("pieces", 711, 0, 1279), ("pieces", 541, 0, 1024), ("pieces", 712, 0, 1281),
         ("distinct_keys", 764, 0, 1535), ("distinct_keys", 460, 0, 1280), ("distinct_keys", 464, 0, 1281),
         ("genome_runs", 575, 0, 1023), ("genome_runs", 1444, 0, 1536), ("genome_runs", 578, 0, 1025),
         ("long_runs", 300, 1, 3), ("long_runs", 300, 2, 4), ("long_runs", 300, 3, 5))
N_NAMED = 32                                               # the records before the random ones


@functools.lru_cache(maxsize=None)
def corpus(n_rand=None, n_long=0):
    """-> (names, ref_len uint32[M], placement, batch = (hits, offsets, p, None)): one read per record.  n_rand: only that many of the
    random records; n_long: as many runs of 20 pieces on wave_more"""
    T, R = _model()
    assert R[N_NAMED - 1][0] == "long_model" and R[N_NAMED][0] == "rand0"
    if n_rand is not None:
        R = R[:N_NAMED + n_rand]
    R = R + [("wave_more", 20 * j, 20, 0.5 if j % 2 == 0 else 0.25) for j in range(n_long)]
    names = [x[0].encode() for x in T]
    tid = {x[0]: i for i, x in enumerate(T)}
    ref_len = np.array([x[1] for x in T], np.uint32)
    off, starts, lens = [0], [], []
    for _, _, status, _, strand, blocks in T:
        for gs, n in (blocks if strand >= 0 else blocks[::-1]):
            starts.append(gs); lens.append(n)
        off.append(len(starts))
    placement = Placement(np.array([x[2] for x in T], np.uint8), np.array([x[3] for x in T], np.int32), np.array([x[4] for x in T], np.int8),
                          np.array(off, np.int64), np.array(starts, np.uint32), np.array(lens, np.uint32), len(CHROM_NAMES), CHROM_NAMES)
    hits, p = np.zeros(len(R), HIT_DTYPE), np.zeros(len(R))
    for i, (name, pos, n, pv) in enumerate(R):
        hits[i]["tid"], hits[i]["pos"], hits[i]["read_len"], hits[i]["fwd"] = tid[name], pos, n, 1
        p[i] = pv
    offsets = np.arange(len(R) + 1, dtype=np.uint32)
    for a in (ref_len, hits, p, offsets) + tuple(placement[:6]):
        a.setflags(write=False)
    return names, ref_len, placement, (hits, offsets, p, None)


def tid(name):
    return corpus()[0].index(name.encode())


@functools.lru_cache(maxsize=None)
def transcript_runs(n_rand=None, n_long=0):
    """hits.coverage_host's runs of the corpus' records: what the projection reads"""
    from sailfish_amd import hits as H
    _, ref_len, _, batch = corpus(n_rand, n_long)
    runs, _, _ = H.coverage_host(ref_len, [batch])
    for a in runs:
        a.setflags(write=False)
    return runs


def big_runs():
    """transcript_runs() with big_a's and big_b's runs of (2^31 - 1) 2^32 put in their places (CPU only)"""
    t, a, b, s = (x.tolist() for x in transcript_runs())
    rows = sorted(list(zip(t, a, b, s)) + [(tid("big_a"), 0, 10, ((1 << 31) - 1) << 32), (tid("big_b"), 2, 8, ((1 << 31) - 1) << 32)])
    return tuple(np.array(col, dt) for col, dt in zip(zip(*rows), (np.uint32, np.uint32, np.uint32, np.uint64)))


@functools.lru_cache(maxsize=None)
def expected(big=False):
    """hits.coverage_genome_host over the corpus -> (runs, stats); computed once, never changed"""
    from sailfish_amd import hits as H
    _, ref_len, placement, _ = corpus()
    t_runs = big_runs() if big else transcript_runs()
    runs, st = H.coverage_genome_host(t_runs, placement, ref_len)
    for a in runs:
        a.setflags(write=False)
    return runs, st


def counts(n_rand, n_long):
    """-> (transcript runs, pieces, distinct keys, genome runs, long runs) of an edge corpus, by the statement"""
    from sailfish_amd import hits as H
    _, ref_len, placement, _ = corpus(n_rand, n_long)
    t_runs = transcript_runs(n_rand, n_long)
    runs, st = H.coverage_genome_host(t_runs, placement, ref_len, with_distinct=True)
    return runs, st


@functools.lru_cache(maxsize=None)
def edge_expected(what, n_rand, n_long, want):
    """the statement's (runs, stats) of the edge corpus (n_rand, n_long), after asserting that its count `what` is `want`"""
    runs, st = counts(n_rand, n_long)
    got = dict(transcript_runs=len(transcript_runs(n_rand, n_long)[0]), pieces=st["n_pieces"], distinct_keys=st["n_distinct"], genome_runs=st["n_runs"],
               long_runs=st["n_long"])[what]
    assert got == want, (what, n_rand, n_long, got, want)
    for a in runs:
        a.setflags(write=False)
    return runs, st
