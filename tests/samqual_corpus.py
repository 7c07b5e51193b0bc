"""Batches with qualities for the tests of the oriented, quality-keeping SAM / BAM writer (tests/test_samqual_cpu.py,
tests/test_gpu_samqual.py).  A case is a dict as in tests/samwrite_corpus.py with one more key: quals, per read the quality bytes
(single end) or a (mate 1, mate 2) pair, a member None where that mate's qualities are not given.

`dress(case, seed)` keeps a case's records, names and SEQ lengths and draws the bases anew from every byte samw_comp knows, in both
cases, plus a few it leaves alone, and the qualities from all of '!' .. '~'.  A read of ONE base never gets the quality '*': in SAM
text that reads as "no qualities", so sam_to_bam of the text and the records the writer makes would differ there by the format's
own ambiguity, which the writer documents and does not resolve.
`reversed_runs(paired, names, ref_len)` holds the reversed runs at every length where the kernels take another path: 0, 1, 2, the
short-copy bound (47, 48, 49), one tile (4095, 4096, 4097) and three tiles (9000), odd and even, on all four strand combinations
of a pair, on reverse orphans of either mate, on secondary records, next to record-less reads (never reversed)."""
import numpy as np

import samwrite_corpus as sw

BASES = np.frombuffer(b"ACGTNacgtnURYKMBDHSWVurykmbdhswv" + b".-=xXZ@", np.uint8)
QUALS = np.arange(33, 127, dtype=np.uint8)
RUNS = [0, 1, 2, 47, 48, 49, 4095, 4096, 4097, 9000]
# what the test's own transform complements (written out again here, not imported from the package)
COMP = bytes.maketrans(b"ATCGURYKMBVDHatcgurykmbvdh", b"TAGCAYRMKVBHDtagcayrmkvbhd")
MODES = [(True, True), (True, False), (False, True), (False, False)]        # (quals, oriented); the last is the old entries' text


def _bases(rng, n):
    return rng.choice(BASES, n).tobytes()


def _quals(rng, n):
    q = rng.choice(QUALS, n).tobytes()
    return b"I" if q == b"*" else q


def dress(case, seed=0, mates=(True, True)):
    """the case with bases of the wide alphabet and qualities; mates: which mate's qualities are given (paired)"""
    rng = np.random.default_rng(9000 + seed)
    seqs, quals = [], []
    for s in case["seqs"]:
        if case["paired"]:
            b = tuple(_bases(rng, len(x)) for x in s)
            seqs.append(b)
            quals.append(tuple(_quals(rng, len(x)) if m else None for x, m in zip(b, mates)))
        else:
            seqs.append(_bases(rng, len(s)))
            quals.append(_quals(rng, len(s)))
    return dict(case, seqs=seqs, quals=quals)


def reversed_runs(paired, names=sw.NAMES, ref_len=sw.REF_LEN):
    rng = np.random.default_rng(77)
    reads = []
    for i, n in enumerate(RUNS):
        m = n + 1 if n else 3                              # the other mate: the other parity
        name = b"run%d" % n + b"x" * (i * 7 % 23)          # the lines start at varying offsets within their tiles
        if paired:
            recs = [sw.rec(i % 6, 10 + i, 200 + i, 300, n, m, f, mf, 3) for f in (0, 1) for mf in (0, 1)]
            recs += [sw.rec(3, 5, 0, 0, n, 0, 0, 0, 1), sw.rec(4, 6, 0, 0, m, 0, 0, 0, 2), sw.rec(4, 6, 0, 0, m, 0, 1, 0, 2)]
            reads.append((name, (_bases(rng, n), _bases(rng, m)), recs))
            reads.append((name + b"/u", (_bases(rng, m), _bases(rng, n)), []))
            reads.append((name + b"/o", (_bases(rng, m), _bases(rng, n)), [sw.rec(5, 7, 0, 0, n, 0, 0, 0, 2)]))
        else:
            reads.append((name, _bases(rng, n), [sw.rec(i % 6, 10 + i, 0, 0, n, 0, f, 0, 0) for f in (0, 1, 0)]))
            reads.append((name + b"/u", _bases(rng, m), []))
            reads.append((name + b"/o", _bases(rng, m), [sw.rec(5, 7, 0, 0, m, 0, 0, 0, 0)]))
    case = dict(sw._case(paired, reads), names=names, ref_len=ref_len)
    quals = [tuple(_quals(rng, len(x)) for x in s) if paired else _quals(rng, len(s)) for s in case["seqs"]]
    return dict(case, quals=quals)


def only(case, mate):
    """the paired case with the qualities of `mate` (0 or 1) alone"""
    return dict(case, quals=[tuple(q if m == mate else None for m, q in enumerate(k)) for k in case["quals"]])


def expected(case, quals, oriented, first_read=0, header=False):
    """samfile._sam_text for the case (its alignment lines, unless header) with or without its qualities, oriented or not"""
    from sailfish_amd import samfile
    n = len(case["offsets"]) - 1
    names = case["read_names"]
    if names is None and first_read:
        names = [b"r%d" % (first_read + r) for r in range(n)]
    text = samfile._sam_text(case["names"], case["ref_len"], case["hits"], case["offsets"], names, case["seqs"],
                             quals=case["quals"] if quals else None, oriented=oriented)
    head = samfile.sam_header(case["names"], case["ref_len"])
    assert text.startswith(head)
    return text if header else text[len(head):]


def line_owners(case):
    """[(read, mate)] of every alignment line, from the records alone"""
    off, out = case["offsets"].astype(np.int64), []
    for r in range(len(off) - 1):
        st = case["hits"]["mate_status"][off[r]:off[r + 1]].tolist()
        if not st:
            out += [(r, 0), (r, 1)] if case["paired"] else [(r, 0)]
        for s in st:
            out += [(r, 0), (r, 1)] if s == 3 else [(r, 1 if s == 2 else 0)]
    return out


def transformed(case, quals, oriented, first_read=0):
    """the same lines made another way: the text WITHOUT qualities and orientation, then per line the qualities put in and, on a
    0x10 line with SEQ, SEQ replaced by seq.translate(COMP)[::-1] and the quality reversed"""
    plain = expected(case, False, False, first_read)
    lines = plain.split(b"\n")
    assert lines.pop() == b""
    owners = line_owners(case)
    assert len(owners) == len(lines)
    out = []
    for l, (r, m) in zip(lines, owners):
        f = l.split(b"\t")
        assert len(f) == 11 and f[10] == b"*"
        q = None
        if quals:
            q = case["quals"][r][m] if case["paired"] else case["quals"][r]
        rev = oriented and int(f[1]) & 0x10 and f[9] != b"*"
        if rev:
            f[9] = f[9].translate(COMP)[::-1]
        if q is not None:
            f[10] = q[::-1] if rev else q
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out)


def arrays(case):
    """samwrite_corpus.arrays and k1 / k2: the qualities of either mate back to back (None where not given)"""
    a = sw.arrays(case)
    a["k1"] = a["k2"] = None
    if case.get("quals") is not None and case["seqs"] is not None:
        mates = [[k[m] for k in case["quals"]] for m in (0, 1)] if case["paired"] else [list(case["quals"])]
        for m, ks in enumerate(mates):
            if all(k is None for k in ks):
                continue
            assert all(k is not None for k in ks)
            buf = np.frombuffer(b"".join(ks), np.uint8).copy()
            a["k%d" % (m + 1)] = buf if len(buf) else np.zeros(1, np.uint8)
    return a


def failing(paired):
    """[(case, read, record, kind)]: batches whose qualities hold a byte outside '!' .. '~' (kind 6, reported as record 0 of the lowest
    such read) alone and next to records that break kinds 1 and 2: the lowest (read, record) wins, then the lowest kind"""
    st = 3 if paired else 0
    ok = sw.rec(0, 5, 9 if paired else 0, 54 if paired else 0, 4, 4 if paired else 0, 1, 0, st)
    bad_pos = sw.rec(0, -4, 9 if paired else 0, 0, 4, 4 if paired else 0, 1, 0, st)
    bad_tid = sw.rec(len(sw.NAMES), 5, 9 if paired else 0, 54 if paired else 0, 4, 4 if paired else 0, 1, 0, st)
    s = (b"ACGT", b"TTGA") if paired else b"ACGT"
    good = (b"IIII", b"!~!~") if paired else b"I~!I"

    def mk(lists, bad):
        """bad: {read: (mate, byte)}"""
        quals = []
        for r in range(len(lists)):
            k = list(good) if paired else [good]
            if r in bad:
                mate, byte = bad[r]
                k[mate] = k[mate][:2] + bytes([byte]) + k[mate][3:]
            quals.append(tuple(k) if paired else k[0])
        return dict(sw._case(paired, [(b"q%d" % i, s, recs) for i, recs in enumerate(lists)]), quals=quals)

    out = [(mk([[ok], [], [ok, ok], [ok]], {2: (0, 32), 3: (0, 9)}), 2, 0, 6),              # the edge below '!'
           (mk([[ok], [ok], [ok]], {1: (0, 127)}), 1, 0, 6),                                 # the edge above '~'
           (mk([[ok], [], [ok]], {1: (0, 10)}), 1, 0, 6),                                    # a read without records
           (mk([[ok], [bad_pos, ok], [ok]], {1: (0, 32)}), 1, 0, 1),                         # kind 1 at record 0 of the same read
           (mk([[ok], [bad_tid], [ok]], {1: (0, 32)}), 1, 0, 2),
           (mk([[ok], [ok, bad_pos], [ok]], {1: (0, 32)}), 1, 0, 6),                         # ... at a later record: the qualities first
           (mk([[ok, bad_tid], [ok], [ok]], {2: (0, 127)}), 0, 1, 2),                        # kind 2 in an earlier read
           (mk([[ok]] * 400 + [[ok, ok]], {399: (0, 0), 400: (0, 255)}), 399, 0, 6)]
    if paired:
        out += [(mk([[ok], [ok], [ok]], {1: (1, 32)}), 1, 0, 6),                             # mate 2 only
                (mk([[ok], [ok], [ok]], {2: (0, 127), 1: (1, 9)}), 1, 0, 6)]
    return out
