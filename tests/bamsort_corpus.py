"""Batches for the sorted-BAM tests (tests/test_bamsort_cpu.py, tests/test_gpu_bamsort.py) and what the host statements of
csrc/baifmt.h -- samfile.sort_bam_stream / write_bam(sort="coordinate"), samfile.build_bai, samfile.fetch -- say about them.  A case
is a dict: names / ref_len (the references), paired, oriented, batches: a list of dict(hits, offsets, read_names, seqs, quals) as
samfile._sam_text takes them.  The shapes are the smallest at which each rule of the sorted file and of the index can go wrong."""
import struct

import numpy as np

from sailfish_amd.hits import HIT_DTYPE
from samwrite_corpus import rec

NAMES = [b"chrA", b"empty", b"chrB", b"chrC"]          # "empty" never gets a record: a reference without records between two with some
REF_LEN = [100000, 500, 60000, 40000]
W = 16384                                               # a window of the linear index, and the span of a level-5 bin


def _bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), n).tobytes())


def _quals(rng, n):
    return bytes(rng.integers(33, 127, n).astype(np.uint8).tobytes())


def _batch(rng, paired, reads, with_quals=True):
    """reads: [(name or None, [records])]; the bases are made to fit the records' read lengths (csrc/bamwfmt.h's rule 4)"""
    hits = np.array([r for _, recs in reads for r in recs], HIT_DTYPE)
    off = np.concatenate([[0], np.cumsum([len(recs) for _, recs in reads])]).astype(np.uint32)
    seqs, quals = [], []
    for _, recs in reads:
        n1 = recs[0][4] if recs and recs[0][8] != 2 else 40
        n2 = recs[0][5] if recs and recs[0][8] == 3 else recs[0][4] if recs and recs[0][8] == 2 else 30
        s = (_bases(rng, n1), _bases(rng, n2)) if paired else _bases(rng, n1)
        seqs.append(s)
        quals.append((_quals(rng, n1), _quals(rng, n2)) if paired else _quals(rng, n1))
    names = [q for q, _ in reads]
    return dict(hits=hits, offsets=off, read_names=None if names and names[0] is None else names, seqs=seqs, quals=quals if with_quals else None)


def _case(paired, batches, names=NAMES, ref_len=REF_LEN, oriented=True):
    return dict(names=names, ref_len=ref_len, paired=paired, oriented=oriented, batches=batches)


def edges():
    """single end, three batches: ties within and across the batches, the level-5 bin edge (a read ending at 16 383, one starting
    at 16 384, one crossing), bin 4681 recurring behind the crossing read's bin, an untouched window between touched ones, reverse
    strands, record-less reads in every batch"""
    rng = np.random.default_rng(11)
    S = lambda tid, pos, fwd=1, rl=50: rec(tid, pos, 0, 0, rl, 0, fwd, 0, 0)
    batches = []
    for b in range(3):
        reads = [(b"tie%d.%d" % (b, i), [S(0, 100, i & 1)]) for i in range(3)]                      # (0, 100) nine times over
        reads += [(b"none%d" % b, []), (b"tieB%d" % b, [S(2, 7, 0, 20)])]
        if b == 0:
            reads += [(b"ends16383", [S(0, W - 50)]), (b"starts16384", [S(0, W, 0)]), (b"crosses", [S(0, W - 24, 0, 48)]),
                      (b"again4681", [S(0, W - 14, 1, 10)]), (b"clipped", [S(0, -5, 0, 30)])]
        if b == 1:
            reads += [(b"window4", [S(0, 4 * W + 9, 0)]), (b"lastbase", [S(0, REF_LEN[0] - 50)]), (b"multi", [S(3, 39000), S(2, 59000, 0), S(0, 3)])]
        if b == 2:
            reads += [(b"before", [S(0, 99)]), (b"chrC0", [S(3, 0, 0, 1)]), (b"none.last", [])]
        batches.append(_batch(rng, False, reads))
    return _case(False, batches)


def pairs():
    """paired, two batches: mates that sort far apart and onto different sides of other fragments, orphans of either side,
    record-less pairs, a pair on two windows"""
    rng = np.random.default_rng(12)
    P = lambda tid, pos, mpos, fwd=1, mfwd=0, rl=50, ml=60: rec(tid, pos, mpos, max(pos + rl, mpos + ml) - min(pos, mpos), rl, ml, fwd, mfwd, 3)
    O = lambda tid, pos, status, fwd=1, rl=50: rec(tid, pos, 0, 0, rl, 0, fwd, 0, status)
    b0 = [(b"far", [P(2, 50, 30000)]), (b"between1", [P(2, 400, 700)]), (b"swapped", [P(2, 20000, 300, 0, 1)]), (b"nopair", []),
          (b"orph1", [O(0, 16000, 1, 0)]), (b"two", [P(0, W - 30, W + 200), P(3, 5, 900, 0, 1)])]
    b1 = [(b"between2", [P(2, 25000, 26000)]), (b"orph2", [O(0, 16000, 2)]), (b"nopair2", []), (b"tie", [P(2, 50, 30000, 0, 1)]),
          (b"same", [P(0, 77, 77, 1, 0, 50, 50)])]
    return _case(True, [_batch(rng, True, b0), _batch(rng, True, b1)])


def big(n_reads=1500):
    """single end, three batches of default names: a record stream of several members (records straddle them), every reference
    but "empty", strands, qualities, record-less reads, reads with several records"""
    rng = np.random.default_rng(13)
    batches, cut = [], [0, n_reads // 2, n_reads // 2 + 1, n_reads]
    for a, b in zip(cut[:-1], cut[1:]):
        reads = []
        for _ in range(a, b):
            k = int(rng.choice([0, 1, 1, 1, 2, 3]))
            rl = int(rng.choice([36, 75, 100]))
            recs = []
            for _ in range(k):
                tid = int(rng.choice([0, 0, 2, 3]))
                recs.append(rec(tid, int(rng.integers(-10, REF_LEN[tid] - rl)), 0, 0, rl, 0, int(rng.integers(0, 2)), 0, 0))
            reads.append((None, recs))
        batches.append(_batch(rng, False, reads))
    return _case(False, batches)


def many_refs(n_refs=2500):
    """a header of more than one member, records on the first, a middle and the last reference"""
    rng = np.random.default_rng(14)
    S = lambda tid, pos: rec(tid, pos, 0, 0, 25, 0, 1, 0, 0)
    reads = [(b"last", [S(n_refs - 1, 900)]), (b"first", [S(0, 0)]), (b"mid", [S(1200, 50), S(1200, 50)]), (b"none", [])]
    return _case(False, [_batch(rng, False, reads, with_quals=False)], names=[b"ref%04d" % i for i in range(n_refs)], ref_len=[1000] * n_refs, oriented=False)


def single():
    rng = np.random.default_rng(15)
    return _case(False, [_batch(rng, False, [(b"only", [rec(2, 12345, 0, 0, 50, 0, 0, 0, 0)])])])


def nothing():
    """no write at all: header and EOF member, an index of empty references"""
    return _case(False, [])


def cases():
    return dict(edges=edges(), pairs=pairs(), big=big(), many_refs=many_refs(), single=single(), nothing=nothing())


def merged(case, batches=None):
    """the batches as one: dict(hits, offsets, read_names, seqs, quals); default names count over the batches, as the writers' do"""
    bs = case["batches"] if batches is None else batches
    if not bs:
        return dict(hits=np.zeros(0, HIT_DTYPE), offsets=np.zeros(1, np.uint32), read_names=None, seqs=None, quals=None)
    off, names, first = [np.zeros(1, np.int64)], [], 0
    for b in bs:
        n = len(b["offsets"]) - 1
        off.append(b["offsets"][1:].astype(np.int64) + off[-1][-1])
        names += b["read_names"] if b["read_names"] is not None else [b"r%d" % (first + r) for r in range(n)]
        first += n
    return dict(hits=np.concatenate([b["hits"] for b in bs]), offsets=np.concatenate(off).astype(np.uint32), read_names=names,
                seqs=[s for b in bs for s in b["seqs"]], quals=None if bs[0]["quals"] is None else [q for b in bs for q in b["quals"]])


def unsorted_stream(case, batches=None):
    """sam_to_bam of the text of all batches: the inflated file of SamDeviceWriter(format="bam") without sort"""
    from sailfish_amd import samfile
    m = merged(case, batches)
    seqs = m["seqs"] if m["seqs"] is not None or not case["paired"] else []
    return samfile.sam_to_bam(samfile._sam_text(case["names"], case["ref_len"], m["hits"], m["offsets"], m["read_names"], seqs, quals=m["quals"],
                                                oriented=case["oriented"]))


def sorted_stream(case, batches=None):
    """the host statement of the sorted file, inflated"""
    from sailfish_amd import samfile
    return samfile.sort_bam_stream(unsorted_stream(case, batches))


def write_host(case, path, member_bytes=65280):
    """write_bam(sort="coordinate") over the merged batches"""
    from sailfish_amd import samfile
    m = merged(case)
    if not case["batches"]:
        m["seqs"] = []                                  # (no batch: _sam_text reads the library off the records, there are none)
    samfile.write_bam(path, case["names"], case["ref_len"], m["hits"], m["offsets"], read_names=m["read_names"], seqs=m["seqs"], quals=m["quals"],
                      oriented=case["oriented"], sort="coordinate", member_bytes=member_bytes)


def records(stream):
    """[(refID, beg, end, bytes)] of an inflated BAM stream"""
    from sailfish_amd import samfile
    p, out = samfile._bam_header(stream)[2], []
    while p < len(stream):
        size, ref, pos, l_name, _mq, _bin, n_cigar = struct.unpack_from("<iiiBBHH", stream, p)
        span = sum(w >> 4 for w in struct.unpack_from("<%dI" % n_cigar, stream, p + 36 + l_name) if w & 15 in (0, 2, 3, 7, 8))
        out.append((ref, pos, pos + max(span, 1), stream[p:p + 4 + size]))
        p += 4 + size
    return out


def brute_force(recs, tid, beg, end):
    """the records on tid that overlap [beg, end), in file order"""
    return [r for ref, b0, b1, r in recs if ref == tid and b0 < end and b1 > max(beg, 0) and max(beg, 0) < end]


def regions(case):
    """a grid of (tid, beg, end): whole references, single bases, regions that end and begin at multiples of 16 384, regions
    without records, empty regions, every reference with and without records (of a long list: the first, the last, two inside)"""
    n = len(case["names"])
    tids = range(n) if n <= 8 else sorted({0, 1, n // 2 - 50, 1200, n - 2, n - 1})
    out = []
    for t in tids:
        L = case["ref_len"][t]
        out += [(t, 0, L), (t, 0, 1), (t, L - 1, L), (t, 0, 2 ** 29), (t, 5, 5), (t, 101, 100), (t, 100, 101), (t, 149, 150), (t, 150, 151)]
        for k in (1, 2, 3, 4, 5):
            out += [(t, k * W - 1, k * W), (t, k * W, k * W + 1), (t, (k - 1) * W, k * W), (t, k * W, (k + 1) * W), (t, k * W - 40, k * W + 40)]
        out += [(t, a, a + 700) for a in range(0, min(L, 70000), 4999)]
    return out
