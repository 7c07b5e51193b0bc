"""The shared corpus of the genome alignment tests (tests/test_galn_cpu.py, tests/test_gpu_galn.py): one exon model, built as
genes.ExonModel.for_names returns it, and two batches that hold every edge of csrc/galnfmt.h's rule, each on a transcript of its own.

GAPPED (a paired library; alignments, nm and MD given; the reads' bases fit the CIGARs, so the writers take it):
  inside                 10M inside block 0: unchanged but for the position
  j_plus / j_minus       blocks of 10 bases with introns of 10, on + and on -: 10M from 5 crosses one junction (5M10N5M); 5M5M from 5
                         (a word that ends exactly at a block's end: no cut, the N follows); 10M from 0 (the line ends there: no N);
                         6M4D6M (a D crossing the junction), 6M2D6M (ending at it), 8M2D6M (starting at it); 5M3I5M (the I stays
                         upstream of the N); on -: 3S12M2S (the clips swap)
  onebase                four 1-base exons: 4M crosses three junctions
  touch                  blocks that touch: 10M over both, no N
  md_minus / md_plus     one block of 200: the MDs 100, 0A99, 10A0C5, 50^AC50 and 5^AC0T3, reversed on - and copied on +
  far                    a block at 4 000 000 000: off_range
  st1 .. st4, noblocks   transcripts that are not placed
  a slot without operations, and a line of soft clips only: unalignable; a position below 0: off_range
  reads: one that loses both its records, one that loses its first (the next one loses 0x100), one that loses a middle record
  pair_plus / pair_minus mates in different blocks (TLEN spans the intron), on - with pos > mate_pos; orphans of mate 1 and of mate 2
  rand0 .. rand7         isoforms over one region on both strands with 300 random records, CIGARs and MDs
UNGAPPED (single end, no alignments: the writer's <clip>S<match>M):
  a negative pos on + and on - (3S7M; on - the clip goes to the end); columns beyond L on + (kept, counted), on - down to 0 (kept) and
  one below (off_range); hi_end: a block that ends at 2^31 - 1 -- a line that ends there is kept, one column further is not; far;
  every status; no base on the transcript (unalignable); 0 bases; random records, some hanging over either end

EDGE corpora: GAPPED's named records, 100 random ones and fillers, so that each count a grid or a scan is sized by -- the records,
the kept lines, the output words and the MD bytes -- falls one below, on and one above a multiple of the 256 lanes of a block.
"""
import collections
import functools

import numpy as np

HIT_DTYPE = np.dtype([("tid", "<u4"), ("pos", "<i4"), ("mate_pos", "<i4"), ("frag_len", "<u4"), ("read_len", "<u2"), ("mate_len", "<u2"), ("fwd", "u1"),
                      ("mate_fwd", "u1"), ("mate_status", "u1"), ("pad_", "u1")])
Placement = collections.namedtuple("Placement", "status chrom strand exon_off exon_start exon_len n_chrom chrom_names")
CHROM_NAMES = [b"chr1", b"chr2", b"chrX"]
CHROM_LENGTHS = [(1 << 31) - 1, (1 << 31) - 1, 50_000]
FAR = 4_000_000_000
HI = (1 << 31) - 1
BLOCK = 256
OPS = "MIDNSHP=X"
N_RAND = 300


def words(cigar):
    """'5M3I5M' -> [len << 4 | op]"""
    out, n = [], ""
    for ch in cigar:
        if ch.isdigit():
            n += ch
        else:
            out.append(int(n) << 4 | OPS.index(ch)); n = ""
    return out


def cigar(ws):
    return "".join("%d%s" % (int(w) >> 4, OPS[int(w) & 15]) for w in ws)


def query_len(ws):
    return sum(w >> 4 for w in ws if (w & 15) in (0, 1, 4, 7, 8))


def ref_len(ws):
    return sum(w >> 4 for w in ws if (w & 15) in (0, 2, 3, 7, 8))


def _transcripts():
    """(name, status, chrom, strand, blocks ascending along the genome)"""
    rng = np.random.default_rng(41)
    T = [("inside", 0, 0, 1, [(100, 50), (200, 30), (300, 40)]),
         ("j_plus", 0, 0, 1, [(1000, 10), (1020, 10), (1040, 10)]),
         ("j_minus", 0, 0, -1, [(2000, 10), (2020, 10), (2040, 10)]),
         ("onebase", 0, 1, 1, [(200, 1), (202, 1), (204, 1), (206, 1)]),
         ("touch", 0, 0, 1, [(7000, 10), (7010, 10)]),
         ("md_minus", 0, 2, -1, [(30000, 200)]),
         ("md_plus", 0, 2, 1, [(31000, 200)]),
         ("far", 0, 1, 1, [(FAR, 60)]),
         ("noblocks", 0, 0, 1, []),
         ("pair_plus", 0, 0, 1, [(10000, 50), (10100, 50)]),
         ("pair_minus", 0, 0, -1, [(11000, 50), (11100, 50)]),
         ("beyond_plus", 0, 0, 1, [(8000, 30)]),
         ("beyond_minus", 0, 0, -1, [(5, 30)]),
         ("hi_end", 0, 0, 1, [(HI - 50, 50)])]
    T += [(f"st{s}", s, -1, 0, []) for s in (1, 2, 3, 4)]
    exons = [(20000 + 150 * i, int(rng.integers(20, 61))) for i in range(30)]
    for k in range(8):
        mine = [e for e in exons if rng.random() < 0.5] or exons[:1]
        T.append((f"rand{k}", 0, 1, 1 if k % 2 == 0 else -1, mine))
    return T


@functools.lru_cache(maxsize=None)
def model():
    """-> (names, placement)"""
    T = _transcripts()
    off, starts, lens = [0], [], []
    for _, _, _, strand, blocks in T:
        for gs, n in (blocks if strand >= 0 else blocks[::-1]):
            starts.append(gs); lens.append(n)
        off.append(len(starts))
    pl = Placement(np.array([x[1] for x in T], np.uint8), np.array([x[2] for x in T], np.int32), np.array([x[3] for x in T], np.int8),
                   np.array(off, np.int64), np.array(starts, np.uint32), np.array(lens, np.uint32), len(CHROM_NAMES), CHROM_NAMES)
    for a in pl[:6]:
        a.setflags(write=False)
    return [x[0].encode() for x in T], pl


def tid(name):
    return model()[0].index(name.encode())


def total_len(name):
    return sum(n for _, n in _transcripts()[tid(name)][4])


def _random_md(rng, n):
    """some MD over about n columns: numbers, letters and deletions in the grammar the reversal reads"""
    out, left = b"", n
    while left > 0:
        run = int(rng.integers(0, left + 1))
        out += b"%d" % run
        left -= run
        if left <= 0:
            return out
        kind = rng.random()
        if kind < 0.6:
            out += bytes([b"ACGTN"[int(rng.integers(0, 5))]])
            left -= 1
        else:
            out += b"^" + bytes(b"ACGTN"[int(x)] for x in rng.integers(0, 5, int(rng.integers(1, 4))))
    return out + b"0"


def _random_cigar(rng, span):
    """S? (M | I | D)+ S? covering about `span` reference columns"""
    ws = []
    if rng.random() < 0.3:
        ws.append(int(rng.integers(1, 6)) << 4 | 4)
    left, first = span, True
    while left > 0:
        n = int(rng.integers(1, min(left, 25) + 1))
        ws.append(n << 4 | (0 if first or rng.random() < 0.7 else 2 if rng.random() < 0.5 else 7))
        left -= n
        first = False
        if left > 0 and rng.random() < 0.3:
            ws.append(int(rng.integers(1, 4)) << 4 | 1)
    if ws[-1] & 15 == 2:
        ws.append(3 << 4)
    if rng.random() < 0.3:
        ws.append(int(rng.integers(1, 6)) << 4 | 4)
    return ws


def _gapped_reads(n_rand, fillers):
    """-> list of reads; a read is a list of records (transcript, mate_status, fwd, mate_fwd, [(x0, words, nm, md) per line])"""
    one = lambda t, x0, c, md=None, st=1, fwd=1, nm=0: (t, st, fwd, 0, [(x0, words(c) if c is not None else [], nm, md if md is not None else b"%d" % ref_len(words(c or "0M")))])      # noqa: E731
    reads = [[one("inside", 5, "10M")],
             [one("j_plus", 5, "10M")], [one("j_minus", 5, "10M", fwd=0)],
             [one("j_plus", 5, "5M5M")], [one("j_minus", 5, "5M5M", st=2)],
             [one("j_plus", 0, "10M")], [one("j_minus", 0, "10M")],
             [one("j_plus", 2, "6M4D6M", b"6^ACGT6", nm=4)], [one("j_minus", 2, "6M4D6M", b"6^ACGT6", nm=4)],
             [one("j_plus", 2, "6M2D6M", b"6^AC6", nm=2)], [one("j_minus", 2, "6M2D6M", b"6^AC6", nm=2)],
             [one("j_plus", 2, "8M2D6M", b"8^AC6", nm=2)], [one("j_minus", 2, "8M2D6M", b"8^AC6", nm=2)],
             [one("j_plus", 5, "5M3I5M", b"10", nm=3)], [one("j_minus", 5, "5M3I5M", b"10", nm=3)],
             [one("j_minus", 0, "3S12M2S", b"12")], [one("j_plus", 0, "3S12M2S", b"12", st=2, fwd=0)],
             [one("onebase", 0, "4M")],
             [one("touch", 5, "10M")]]
    for t in ("md_minus", "md_plus"):
        reads += [[one(t, 7, "100M", b"100")], [one(t, 7, "100M", b"0A99", nm=1)], [one(t, 7, "17M", b"10A0C5", nm=2)],
                  [one(t, 7, "50M2D50M", b"50^AC50", nm=2)], [one(t, 7, "5M2D4M", b"5^AC0T3", nm=3)]]
    reads += [[one("far", 0, "10M")], [one("noblocks", 0, "10M")],
              [one("inside", 0, None)],                     # a slot without operations
              [one("inside", 3, "10S")],                    # no reference column
              [one("inside", -1, "10M")],                   # a position below 0
              [one("st1", 0, "10M"), one("st2", 0, "10M")],                            # loses both
              [one("st3", 0, "10M"), one("inside", 20, "10M")],                        # loses its first
              [one("inside", 30, "10M"), one("st4", 0, "10M"), one("j_plus", 5, "10M")],       # loses a middle one
              [("pair_plus", 3, 1, 0, [(5, words("30M"), 0, b"30"), (60, words("30M"), 1, b"3A26")])],
              [("pair_minus", 3, 1, 0, [(5, words("30M"), 0, b"30"), (60, words("30M"), 1, b"3A26")])],
              [("pair_plus", 3, 0, 1, [(40, words("30M"), 0, b"30"), (0, words("2S20M"), 0, b"20")])],     # line 0 crosses, pos > mate_pos
              [("pair_minus", 3, 1, 0, [(5, words("30M"), 0, b"30"), (0, [], 0, b"")])],                   # a pair falls with one line
              [("pair_plus", 3, 1, 0, [(5, words("30M"), 0, b"30"), (FAR, words("30M"), 0, b"30")])]]      # ... of either kind
    rng = np.random.default_rng(43)
    for k in range(N_RAND):
        t = f"rand{int(rng.integers(0, 8))}"
        L = total_len(t)
        lines = []
        st = (1, 2, 3)[int(rng.integers(0, 3))]
        for _ in range(2 if st == 3 else 1):
            span = int(rng.integers(5, 80))
            ws = _random_cigar(rng, span)
            lines.append((int(rng.integers(0, max(L - span // 2, 1))), ws, int(rng.integers(0, 5)), _random_md(rng, span)))
        if k < n_rand:
            reads.append([(t, st, int(rng.integers(0, 2)), int(rng.integers(0, 2)), lines)])
    for kind, count in fillers:
        reads += [[one("inside", 1, "10M") if kind == "plain" else one("inside", 1, "100M", b"100") if kind == "md3" else one("st1", 0, "10M")]] * count
    return reads


@functools.lru_cache(maxsize=None)
def gapped(n_rand=N_RAND, fillers=()):
    """-> dict(hits, offsets, alignments=(pos, nm, op_off, ops), tags=(nm, md_off, md), seqs=[(mate 1, mate 2) per read])"""
    reads = _gapped_reads(n_rand, fillers)
    rng = np.random.default_rng(47)
    n = sum(len(r) for r in reads)
    hits = np.zeros(n, HIT_DTYPE)
    off, pos, nm, op_cnt, ops, md_cnt, md, seqs = [0], [], [], [], [], [], [], []
    i = 0
    for recs in reads:
        lens = [10, 10]                                   # the read's mates: every record of a read names the same two
        for t, st, fwd, mfwd, lines in recs:
            h = hits[i]
            h["tid"], h["mate_status"], h["fwd"], h["mate_fwd"] = tid(t), st, fwd, mfwd
            h["pos"], h["read_len"] = lines[0][0] if abs(lines[0][0]) < 1 << 31 else 0, query_len(lines[0][1])
            lens[1 if st == 2 else 0] = query_len(lines[0][1]) or 10
            if st == 3:
                h["mate_pos"], h["mate_len"] = lines[1][0] if lines[1][0] < 1 << 31 else 0, query_len(lines[1][1])
                h["frag_len"] = 77
                lens[1] = query_len(lines[1][1]) or 10
            for j in range(2):
                x0, ws, m, text = lines[j] if j < len(lines) else (0, [], 0, b"")
                pos.append(x0 if x0 < 1 << 31 else HI - 5); nm.append(m); op_cnt.append(len(ws)); ops += ws; md_cnt.append(len(text)); md.append(text)
            i += 1
        off.append(i)
        seqs.append(tuple(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), k)) for k in lens))
    csr = lambda c: np.concatenate([[0], np.cumsum(np.array(c, np.uint64), dtype=np.uint64)]).astype(np.uint64)      # noqa: E731
    out = dict(hits=hits, offsets=np.array(off, np.uint32), alignments=(np.array(pos, np.int32), np.array(nm, np.uint32), csr(op_cnt), np.array(ops, np.uint32)),
               tags=(np.array(nm, np.uint32), csr(md_cnt), np.frombuffer(b"".join(md), np.uint8)), seqs=seqs)
    for a in (out["hits"], out["offsets"]) + out["alignments"] + out["tags"]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ungapped():
    """-> dict(hits, offsets): single end, one read per record but for the last reads, which hold several"""
    R = [("inside", -3, 10, 1), ("j_minus", -3, 20, 0), ("j_plus", 5, 10, 1), ("j_minus", 5, 10, 1), ("onebase", 0, 4, 1), ("touch", 5, 10, 0),
         ("beyond_plus", 20, 20, 1), ("beyond_plus", 35, 5, 1), ("beyond_minus", 25, 10, 1), ("beyond_minus", 26, 10, 1), ("beyond_minus", 30, 5, 0),
         ("hi_end", 40, 10, 1), ("hi_end", 41, 10, 1), ("hi_end", 50, 1, 1), ("far", 0, 10, 1), ("noblocks", 0, 10, 1),
         ("inside", -10, 10, 1), ("inside", -11, 10, 1), ("inside", 5, 0, 1), ("st1", 0, 10, 1), ("st2", 0, 10, 1), ("st3", 0, 10, 1), ("st4", 0, 10, 1)]
    rng = np.random.default_rng(53)
    for _ in range(300):
        t = f"rand{int(rng.integers(0, 8))}"
        n = int(rng.integers(20, 61))
        R.append((t, int(rng.integers(-15, total_len(t) + 5)), n, int(rng.integers(0, 2))))
    hits = np.zeros(len(R), HIT_DTYPE)
    for i, (t, p, n, fwd) in enumerate(R):
        hits[i]["tid"], hits[i]["pos"], hits[i]["read_len"], hits[i]["fwd"] = tid(t), p, n, fwd
    off = list(range(len(R) - 8)) + [len(R) - 8, len(R) - 8, len(R) - 5, len(R)]        # ... then an empty read, one of three and one of five
    out = dict(hits=hits, offsets=np.array(off, np.uint32))
    hits.setflags(write=False); out["offsets"].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(which):
    """project_alignments_host over GAPPED ("gapped"), over GAPPED without its tags ("untagged") or over UNGAPPED ("ungapped"): computed
    once, never changed"""
    from sailfish_amd import hits as H
    pl = model()[1]
    if which == "ungapped":
        b = ungapped()
        return H.project_alignments_host(b["hits"], b["offsets"], pl)
    b = gapped()
    return H.project_alignments_host(b["hits"], b["offsets"], pl, b["alignments"], b["tags"] if which == "gapped" else None)


COUNTS = ("records", "kept_lines", "words_out", "md_bytes")


def _counts(batch, res):
    return dict(records=len(batch["hits"]), kept_lines=res[5]["lines"], words_out=res[5]["words_out"], md_bytes=len(res[3][2]))


@functools.lru_cache(maxsize=None)
def edge(what, delta):
    """the edge corpus whose count `what` is a multiple of 256 plus delta -> (batch, the statement's result)"""
    from sailfish_amd import hits as H
    pl = model()[1]
    base = gapped(100)
    have = _counts(base, H.project_alignments_host(base["hits"], base["offsets"], pl, base["alignments"], base["tags"]))[what]
    target = BLOCK * ((have + 8) // BLOCK + 1) + delta
    need = target - have
    if what == "records":
        fillers = (("dropped", need),)
    elif what == "md_bytes":                               # a plain filler's MD is "10", an md3 filler's "100"
        fillers = (("md3", need % 2), ("plain", (need - 3 * (need % 2)) // 2))
    else:
        fillers = (("plain", need),)
    b = gapped(100, fillers)
    res = H.project_alignments_host(b["hits"], b["offsets"], pl, b["alignments"], b["tags"])
    assert _counts(b, res)[what] == target and target % BLOCK == delta % BLOCK, (what, delta, _counts(b, res), target)
    return b, res


EDGES = [(what, d) for what in COUNTS for d in (-1, 0, 1)]


# ---- the spliced genome of the end-to-end test ---------------------------------------------------------------------------------
GENOME_SEED = 439


@functools.lru_cache(maxsize=None)
def genome(seed=GENOME_SEED):
    """three chromosomes, six genes of three isoforms on both strands, exons of 40 to 120 bases; 300 error-free inward pairs of 2 x 40
    -> (names, transcripts, mate 1, mate 2, the GTF's bytes, {chromosome: bases})"""
    import rescue_corpus
    rng = np.random.default_rng(seed)
    chroms = {b"chrB": rescue_corpus.rand(rng, 3000), b"chrA": rescue_corpus.rand(rng, 2500), b"chr10": rescue_corpus.rand(rng, 2500)}
    names, seqs, gtf = [], [], [b"# a spliced genome\n"]
    for gi, (c, strand, at) in enumerate(((b"chrB", b"+", 100), (b"chrB", b"-", 1500), (b"chrA", b"+", 50), (b"chrA", b"-", 1200), (b"chr10", b"+", 200),
                                          (b"chr10", b"-", 1000))):
        exons = []
        for _ in range(5):
            n = int(rng.integers(40, 121))
            exons.append((at, n))
            at += n + int(rng.integers(30, 90))
        for ii, keep in enumerate(((0, 1, 2, 3, 4), (0, 2, 4), (1, 2, 3))):
            name = b"g%d.i%d" % (gi, ii)
            s = b"".join(chroms[c][exons[k][0]:exons[k][0] + exons[k][1]] for k in keep)
            names.append(name.decode()); seqs.append(s if strand == b"+" else rescue_corpus.revcomp(s))
            for k in keep[::-1] if ii == 1 else keep:      # (the file's order of a transcript's exons does not matter)
                gtf.append(b'%s\ttest\texon\t%d\t%d\t.\t%s\t.\tgene_id "g%d"; transcript_id "%s";\n' % (c, exons[k][0] + 1, exons[k][0] + exons[k][1], strand, gi, name))
    r1, r2, _ = rescue_corpus.fragments(rng, seqs, 300, 40, frag_mean=130, frag_sd=15)
    return names, seqs, r1, r2, b"".join(gtf), chroms
