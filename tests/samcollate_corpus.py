"""SAM texts whose lines stand in any order, shared by test_samcollate_cpu.py (samcfmt.h serially, no GPU) and
test_gpu_samcollate.py (the device reader with collate=True): names that try the exact name sort, fragments scattered through the
file, pairing by mate fields, malformed mate fields, and position-sorted / shuffled forms of random hit batches.  Transcripts,
header and the `paired` convention are sam_corpus's: the single-end form of a text is the same lines with the pairing bits taken
out of every FLAG."""
import random

import numpy as np

import sam_corpus as base

NAMES, REF_LEN, PAIR_BITS = base.NAMES, base.REF_LEN, base.PAIR_BITS
BAD_NUMBER, BAD_QNAME = 2, 64


def header(order=b"coordinate"):
    return base.header().replace(b"SO:unsorted", b"SO:" + order)


def line(paired, q, flag, t=None, pos=0, cigar=b"50M", rnext=b"*", pnext=0, seq=b"*", eol=b"\n"):
    """one alignment line; rnext may be b"=", b"*", or a transcript index"""
    if not paired:
        flag &= ~PAIR_BITS
    rname = b"*" if t is None else NAMES[t]
    if isinstance(rnext, int):
        rnext = NAMES[rnext]
    if isinstance(pnext, int):
        pnext = b"%d" % pnext
    return b"\t".join([q, b"%d" % flag, rname, b"%d" % pos, b"255", b"*" if t is None else cigar, rnext, pnext, b"0", seq, b"*"]) + eol


def mates(paired, q, t, p1, p2, sec=0, c1=b"50M", c2=b"50M"):
    """the two lines of a proper pair, each naming the other: -> (line of mate 1, line of mate 2)"""
    return (line(paired, q, 99 | sec, t, p1, c1, b"=", p2), line(paired, q, 147 | sec, t, p2, c2, b"=", p1))


# ---- 1. names -----------------------------------------------------------------------------------------------------------------

def tricky_names():
    """lengths 1, 7, 8, 9, 16, 17 and 254; prefixes of one another; names equal in their first 8, 16 and 24 bytes that differ in the
    last byte; '*'; non-ASCII bytes; names that differ by a trailing or an inner NUL"""
    out = [b"x" * n for n in (1, 7, 8, 9, 16, 17, 254)]
    out += [b"r1", b"r10", b"r100"]
    for n in (8, 16, 24):
        out += [b"s" * n + b"A", b"s" * n + b"B"]
    out += [b"s" * 7 + b"A", b"s" * 7 + b"B", b"s" * 15 + b"A", b"s" * 15 + b"B"]      # the last byte is the last of a round
    out += [b"*", b"\xff\xfe read", b"\xc3\xa9", b"n\x00", b"n", b"n\x00\x00", b"y" * 253 + b"A", b"y" * 253 + b"B"]
    assert len(set(out)) == len(out)
    return out


def names_file(paired, seed=5):
    """every tricky name is a fragment of one pair and one unmapped extra line; the lines are shuffled, so no two lines of a name
    follow each other"""
    rng = random.Random(seed)
    lines = []
    for i, q in enumerate(tricky_names()):
        a, b = mates(paired, q, i % 5, 10 + i, 200 + i)
        lines += [a, b, line(paired, q, 77 | 0x100)]
    rng.shuffle(lines)
    return header(b"unsorted") + b"".join(lines)


def long_qname(paired):
    """a 255-byte QNAME in front of a line that breaks nothing else -> (text, kind, 1-based line)"""
    pre = header() + b"".join(mates(paired, b"ok", 0, 5, 105))
    bad = line(paired, b"q" * 255, 73, 1, 7, b"50M")
    return pre + bad + b"".join(mates(paired, b"ok2", 0, 6, 106)), BAD_QNAME, pre.count(b"\n") + 1


# ---- 2. fragments scattered through the file ----------------------------------------------------------------------------------

def scattered(paired):
    """one fragment whose lines lie at the file's beginning, middle and end; one fragment of 3 000 lines (1 500 pairs on six
    transcripts, positions all different) interleaved with 3 000 fragments of one line"""
    out = [header()]
    a, b = mates(paired, b"wide", 2, 40, 900)
    out.append(a)
    big = []
    for i in range(1500):
        t = (6, 4, 3, 2, 1, 0)[i % 6]
        big += list(mates(paired, b"big", t, 1 + i, 501 + i, sec=0x100 if i else 0))
    ones = [line(paired, b"one%d" % i, 73 if i % 2 else 137, i % 5, 1 + i % 700, b"50M") for i in range(3000)]
    for i in range(3000):
        out += [big[i], ones[i]]
        if i == 1500:
            out.append(line(paired, b"wide", 73 | 0x100, 4, 77, b"50M"))       # an orphan: the pair makes it vanish
    out.append(b)
    return b"".join(out)


# ---- 3. pairing by mate fields ------------------------------------------------------------------------------------------------

def pairing(paired):
    """-> (text, {qname: what a paired call must yield, as [(mate_status, tid, pos, mate_pos)]})"""
    L = lambda *a, **k: line(paired, *a, **k)
    out, want = [header()], {}
    # two pairs of one fragment on one transcript, in position order a1 a2 b1 b2: the neighbour rule would pair a2 with b1
    a1, b1 = mates(paired, b"nest", 1, 100, 300)
    a2, b2 = mates(paired, b"nest", 1, 150, 350, sec=0x100)
    out += [a1, a2, b1, b2]
    want[b"nest"] = [(3, 1, 99, 299), (3, 1, 149, 349)]
    # the same with the side-2 lines in front
    a1, b1 = mates(paired, b"nestrev", 2, 100, 300)
    a2, b2 = mates(paired, b"nestrev", 2, 150, 350, sec=0x100)
    out += [b1, b2, a1, a2]
    want[b"nestrev"] = [(3, 2, 99, 299), (3, 2, 149, 349)]
    # one key twice on side 1, once on side 2: one pair (the first side-1 line), and the fragment yields pairs only
    a, b = mates(paired, b"dup", 0, 10, 210)
    out += [a, a.replace(b"\t99\t", b"\t355\t") if paired else a, b, L(b"dup", 73 | 0x100, 4, 5)]
    want[b"dup"] = [(3, 0, 9, 209)]
    # two pairs with ONE key: the i-th side-1 line with the i-th side-2 line (told apart by their read lengths)
    out += [L(b"twice", 99, 3, 20, b"30M", b"=", 220), L(b"twice", 355, 3, 20, b"40M", b"=", 220),
            L(b"twice", 147, 3, 220, b"31M", b"=", 20), L(b"twice", 403, 3, 220, b"41M", b"=", 20)]
    want[b"twice"] = [(3, 3, 19, 219), (3, 3, 19, 219)]
    # mate fields that do not reciprocate: PNEXT off by one -> two orphans, left then right
    out += [L(b"off1", 147, 1, 300, b"50M", b"=", 100), L(b"off1", 99, 1, 100, b"50M", b"=", 301)]
    want[b"off1"] = [(1, 1, 99, 0), (2, 1, 299, 0)]
    # RNEXT names another transcript; RNEXT spelled out equal to RNAME
    out += [L(b"other", 99, 1, 100, b"50M", 2, 300), L(b"other", 147, 1, 300, b"50M", 2, 100)]
    want[b"other"] = [(1, 1, 99, 0), (2, 1, 299, 0)]
    out += [L(b"spelled", 99, 4, 100, b"50M", 4, 300), L(b"spelled", 147, 4, 300, b"50M", b"=", 100)]
    want[b"spelled"] = [(3, 4, 99, 299)]
    # 0x8 set with a plausible PNEXT; PNEXT 0
    out += [L(b"flag8", 99 | 0x8, 1, 100, b"50M", b"=", 300), L(b"flag8", 147, 1, 300, b"50M", b"=", 100)]
    want[b"flag8"] = [(1, 1, 99, 0), (2, 1, 299, 0)]
    out += [L(b"pnext0", 99, 1, 100, b"50M", b"=", 0), L(b"pnext0", 147, 1, 300, b"50M", b"=", 100)]
    want[b"pnext0"] = [(1, 1, 99, 0), (2, 1, 299, 0)]
    # soft-clipped lines match on the written POS; the record carries pos = POS - 1 - 5
    out += [L(b"clip", 99, 6, 1, b"5S45M", b"=", 120), L(b"clip", 147, 6, 120, b"3S47M", b"=", 1)]
    want[b"clip"] = [(3, 6, -5, 116)]
    # a 0x100 pair next to the primary one on another transcript; a 0x800 line between them yields nothing
    a1, b1 = mates(paired, b"sec", 2, 10, 210)
    a2, b2 = mates(paired, b"sec", 0, 30, 230, sec=0x100)
    out += [a2, L(b"sec", 2048 | 99, 0, 400, b"20H30M", b"=", 230), a1, b2, b1]
    want[b"sec"] = [(3, 0, 29, 229), (3, 2, 9, 209)]
    # mates on two transcripts, each naming the other by its name: orphans
    out += [L(b"split", 65, 6, 30, b"50M", 0, 40), L(b"split", 129, 0, 40, b"50M", 6, 30)]
    want[b"split"] = [(1, 6, 29, 0), (2, 0, 39, 0)]
    # unmapped mates at the end of the file, RNAME '*', as samtools sort leaves them; their mate fields are not looked at
    out += [L(b"unm", 77, None, 0, b"*", b"*", 0), L(b"unm", 141, None, 0, b"*", b"*", 0)]
    want[b"unm"] = []
    return b"".join(out), want


# ---- 4. malformed input -------------------------------------------------------------------------------------------------------

def malformed(paired):
    """-> [(name, text, kind or 0, 1-based line)]: PNEXT that is no number on a mapped line (BAD_NUMBER in a paired call, fine in a
    single-end one, and fine on an unmapped line), the lowest bad line across blocks, the 255-byte QNAME, every case of
    sam_corpus.malformed"""
    out = []
    pre = header() + b"".join(b"".join(mates(paired, b"g%d" % i, i % 5, 10 + i, 300 + i)) for i in range(40))
    post = b"".join(b"".join(mates(paired, b"h%d" % i, i % 5, 10 + i, 300 + i)) for i in range(40))
    at = pre.count(b"\n") + 1
    for name, pn in (("pnext_12x", b"12x"), ("pnext_empty", b""), ("pnext_11_digits", b"00000000001"), ("pnext_2_31", b"2147483648")):
        bad = line(paired, b"bad", 99, 1, 100, b"50M", b"=", pn)
        out.append((name, pre + bad + post, BAD_NUMBER if paired else 0, at))
        out.append((name + "_unmapped", pre + line(paired, b"bad", 77, None, 0, b"*", b"*", pn) + post, 0, at))
    # a later line breaks an earlier rule: the lowest line wins, wherever the blocks end
    first = line(paired, b"bad", 99, 1, 100, b"50M", b"=", b"-1") if paired else line(paired, b"q" * 300, 0, 1, 100)
    later = b"short\t0\ttA\n"
    out.append(("lowest_line", pre + first + post + later, BAD_NUMBER if paired else BAD_QNAME, at))
    # PNEXT and QNAME on one line: NUMBER is the earlier rule; RNAME in front of QNAME
    both = line(paired, b"q" * 255, 99, 1, 100, b"50M", b"=", b"z")
    out.append(("number_before_qname", pre + both + post, BAD_NUMBER if paired else BAD_QNAME, at))
    rn = line(paired, b"q" * 255, 99, 1, 100, b"50M", b"=", 5).replace(b"\t" + NAMES[1] + b"\t", b"\tnowhere\t")
    out.append(("rname_before_qname", pre + rn + post, 8, at))
    text, kind, ln = long_qname(paired)
    out.append(("qname_255", text, kind, ln))
    out.append(("qname_255_unmapped", pre + line(paired, b"q" * 255, 77) + post, BAD_QNAME, at))
    out += [(n, t, k, ln) for n, t, k, ln in base.malformed(paired)]
    return out


# ---- 5. random files: position-sorted and shuffled forms of hit batches ----------------------------------------------------------

def random_batch(seed, paired, n_reads=400):
    """-> (hits, offsets, read names): pairs, orphans, multi-mappers and reads without records, no two records of one kind on one
    transcript within a read (asserted): the order inside a fragment then does not depend on the order of its lines"""
    from sailfish_amd.hits import HIT_DTYPE
    rng = random.Random(seed)
    recs, off, names = [], [0], []
    for r in range(n_reads):
        names.append(b"read%d/%d" % (seed, r) if r % 3 else b"r%d" % r)
        kind = rng.random()
        tids = sorted(rng.sample([0, 1, 2, 3, 4, 6], rng.choice([1, 1, 2, 3, 6])))
        if kind < 0.1:
            tids = []
        for t in tids:
            n1, n2 = rng.randrange(20, 120), rng.randrange(20, 120)
            p1, p2 = rng.randrange(-5, 400), rng.randrange(0, 400)
            if not paired:
                recs.append((t, p1, 0, 0, n1, 0, rng.randrange(2), 0, 0, 0))
            elif kind < 0.7:
                recs.append((t, p1, p2, max(p1 + n1, p2 + n2) - min(p1, p2), n1, n2, rng.randrange(2), rng.randrange(2), 3, 0))
            else:                                        # orphans: all left, all right, or (below) left ones in front of right ones
                recs.append((t, p1, 0, 0, n1, 0, rng.randrange(2), 0, 1 if kind < 0.85 else 2, 0))
        if paired and kind >= 0.95 and len(tids) > 1:
            mixed = recs[off[-1]:]
            recs[off[-1]:] = [r[:8] + (1, 0) for r in mixed[::2]] + [r[:8] + (2, 0) for r in mixed[1::2]]
        off.append(len(recs))
    hits = np.array(recs, dtype=HIT_DTYPE)
    offsets = np.array(off, np.uint32)
    for r in range(n_reads):
        seen = [(int(h["mate_status"]), int(h["tid"])) for h in hits[off[r]:off[r + 1]]]
        assert len(set(seen)) == len(seen), "two records of one kind on one transcript in one read"
    return hits, offsets, names


def random_forms(seed, paired):
    """-> (grouped text, position-sorted text, shuffled text) of one random batch: samfile._sam_text, its header kept, its alignment
    lines (a) in (tid, POS) order with the unmapped lines last, as samtools sort leaves them, (b) in a seeded random order"""
    from sailfish_amd import samfile
    hits, off, names = random_batch(seed, paired)
    text = samfile._sam_text(NAMES, REF_LEN, hits, off, names, None)
    lines = text.split(b"\n")[:-1]
    head = [l + b"\n" for l in lines if l.startswith(b"@")]
    body = [l + b"\n" for l in lines if not l.startswith(b"@")]
    tid_of = {n: i for i, n in enumerate(NAMES)}

    def place(l):
        f = l.split(b"\t")
        return (tid_of.get(f[2], len(NAMES)), int(f[3]))
    by_pos = sorted(body, key=place)                      # (sorted is stable, as samtools sort is)
    shuffled = list(body)
    random.Random(seed + 1000).shuffle(shuffled)
    head_sorted = [h.replace(b"SO:unsorted\tGO:query", b"SO:coordinate") for h in head]
    return text, b"".join(head_sorted + by_pos), b"".join(head + shuffled)


def by_name(text, hits, off):
    """the fragments of a reading re-ordered by QNAME: {qname: its records' bytes}; the i-th fragment is the i-th distinct QNAME"""
    order = {}
    for l in text.split(b"\n"):
        if l and not l.startswith(b"@"):
            order.setdefault(l.split(b"\t")[0], len(order))
    assert len(order) == len(off) - 1
    return {q: hits[off[i]:off[i + 1]].tobytes() for q, i in order.items()}


def files(paired):
    """-> [(name, text)]: every well-formed corpus file"""
    out = [("names", names_file(paired)), ("scattered", scattered(paired)), ("pairing", pairing(paired)[0])]
    for seed in (1, 2):
        grouped, by_pos, shuffled = random_forms(seed, paired)
        out += [(f"random{seed}_grouped", grouped), (f"random{seed}_sorted", by_pos), (f"random{seed}_shuffled", shuffled)]
    out += [(n, t) for n, t, k, _ in malformed(paired) if not k]
    out += [("empty", b""), ("header_only", header())]
    return out


def bam_files(paired):
    """-> [(name, SAM text, samfile.sam_to_bam of it)]: every file of files() that BAM can say (a PNEXT that is no number cannot be
    written; an empty text has no BAM header)"""
    from sailfish_amd import samfile
    skip = {"empty"} | {n for n, _, k, _ in malformed(paired) if n.startswith("pnext_") and not n.startswith("pnext_11")}
    return [(n, t, samfile.sam_to_bam(t)) for n, t in files(paired) if n not in skip]
