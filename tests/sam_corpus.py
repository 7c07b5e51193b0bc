"""SAM texts shared by test_sam_cpu.py (samfmt.h serially, no GPU) and test_gpu_sam.py (the device reader): a corner file, one
malformed file per rule, and a seeded random generator.  Every generator takes `paired`: the single-end form of a text is the
same lines with the pairing bits (0x1, 0x2, 0x8, 0x20, 0x40, 0x80) taken out of every FLAG."""
import random

# prefixes of each other, a name with a space and high bytes, and one no line uses
NAMES = [b"tA", b"tA.1", b"tAB", b"t", b"chr 1|\xc3\xa9", b"unused", b"tZ"]
REF_LEN = [1000, 2000, 1500, 800, 3000, 500, 1200]
PAIR_BITS = 0x1 | 0x2 | 0x8 | 0x20 | 0x40 | 0x80


def header(eol=b"\n"):
    return b"@HD\tVN:1.6\tSO:unsorted" + eol + b"".join(b"@SQ\tSN:%s\tLN:%d" % (n, l) + eol for n, l in zip(NAMES, REF_LEN)) + b"@PG\tID:mapper" + eol


def line(paired, q, flag, t=None, pos=0, cigar=b"*", seq=b"*", eol=b"\n", qual=b"*", extra=b""):
    if not paired:
        flag &= ~PAIR_BITS
    rname = b"*" if t is None else NAMES[t]
    return b"\t".join([q, b"%d" % flag, rname, b"%d" % pos, b"255", cigar, b"*", b"0", b"0", seq, qual]) + extra + eol


def m50(n=50):
    return b"%dM" % n


def corner(paired):
    """-> bytes.  What it holds is listed in place; the last line lacks its newline."""
    L = lambda *a, **k: line(paired, *a, **k)
    out = [header()]
    # a proper pair, CRLF line ends, a QNAME with spaces and high bytes
    q = b"read one \xff\xfe"
    out += [L(q, 99, 0, 101, m50(), eol=b"\r\n"), L(q, 147, 0, 251, m50(), eol=b"\r\n")]
    # names that are prefixes of each other: three groups
    out += [L(b"q1", 99, 1, 11, m50()), L(b"q1", 147, 1, 111, m50()),
            L(b"q10", 99, 1, 12, m50()), L(b"q10", 147, 1, 112, m50()),
            L(b"q1", 99, 2, 13, m50()), L(b"q1", 147, 2, 113, m50())]
    # an unmapped read between mapped ones, and a header line in the middle of the file
    out += [L(b"u1", 77), L(b"u1", 141), b"@CO\ta comment between two groups\n"]
    # a pair next to orphans in one group: the orphans vanish; a header line inside the group takes no part in it
    out += [L(b"mix", 73, 4, 5, m50()), L(b"mix", 99, 0, 7, m50()), b"@CO\tinside a group\n", L(b"mix", 147, 0, 300, m50()), L(b"mix", 137 | 0x100, 6, 9, m50())]
    # mate 2 in front of mate 1: no pair, two orphans, the left one first
    out += [L(b"rev", 147, 1, 400, m50()), L(b"rev", 99, 1, 200, m50())]
    # mates on different transcripts: orphans
    out += [L(b"split", 65, 6, 30, m50()), L(b"split", 129, 0, 40, m50())]
    # a same-strand pair, and one whose mates overlap completely
    out += [L(b"same", 67, 3, 10, m50()), L(b"same", 131, 3, 90, m50()), L(b"in", 83, 3, 20, m50(100)), L(b"in", 163, 3, 30, m50(20))]
    # soft and hard clips (the lead counts S behind leading H only), SEQ given, an insertion and a deletion
    out += [L(b"clip", 99, 2, 100, b"2H3S10M1I5M2D29M2S4H", seq=b"A" * 50), L(b"clip", 147, 2, 300, b"3S47M")]
    out += [L(b"hsh", 73, 2, 100, b"5S2H43M")]
    # SEQ * with a CIGAR, CIGAR * with a SEQ, both *: lengths 60, 33, 0
    out += [L(b"star", 99, 0, 500, b"60M"), L(b"star", 147, 0, 600, seq=b"C" * 33), L(b"star0", 73, 0, 1)]
    # a read that begins in front of its transcript: pos = -5
    out += [L(b"neg", 99, 4, 1, b"5S45M"), L(b"neg", 147, 4, 20, b"50M")]
    # secondary lines carry the multi-mappings; a supplementary line yields nothing but belongs to the group
    out += [L(b"multi", 99, 6, 10, m50()), L(b"multi", 147, 6, 110, m50()), L(b"multi", 2147, 6, 500, b"20H30M"),
            L(b"multi", 355, 2, 10, m50()), L(b"multi", 403, 2, 110, m50()), L(b"multi", 355, 6, 20, m50()), L(b"multi", 403, 6, 120, m50()),
            L(b"multi", 355, 0, 10, m50()), L(b"multi", 403, 0, 110, m50())]
    # orphans whose tids arrive descending and duplicated, right ones in front of left ones
    out += [L(b"orph", 137, 6, 1, m50()), L(b"orph", 137 | 0x100, 2, 2, m50()), L(b"orph", 73 | 0x100, 4, 3, m50()),
            L(b"orph", 73 | 0x100, 1, 4, m50()), L(b"orph", 137 | 0x100, 2, 5, m50()), L(b"orph", 73 | 0x100, 4, 6, m50())]
    # only unmapped and supplementary lines: a read with no record
    out += [L(b"none", 77), L(b"none", 141), L(b"none", 2048 | 65, 0, 5, b"40H10M")]
    # one group of 5 000 lines: 2 500 pairs, tids descending and repeating, every position its own
    big = []
    for i in range(2500):
        t = 6 - i % 7 if i % 7 != 1 else 6                   # (5 = "unused" is skipped)
        big += [L(b"big", 99 | (0x100 if i else 0), t, 1 + i, m50()), L(b"big", 147 | (0x100 if i else 0), t, 101 + i, m50())]
    out += big
    # POS at its upper end, a read of 65 535 bases by CIGAR, FLAG with five digits and leading zeros
    out += [L(b"edge", 65, 0, 2 ** 31 - 1, b"65535M"), L(b"edge", 129 | 0x400, 1, 1, b"1M", seq=b"G")]
    out += [line(paired, b"zeros", 0, 3, 7, m50()).replace(b"\t0\t", b"\t00073\t" if paired else b"\t00000\t", 1)]
    # a last line without its newline, with fields behind the eleventh
    out += [L(b"last", 73, 0, 77, m50(), extra=b"\tNH:i:1\tXS:Z:a\tb", eol=b"")]
    return b"".join(out)


def good_group(paired, q, t=0, pos=10):
    return line(paired, q, 99, t, pos, m50()) + line(paired, q, 147, t, pos + 100, m50())


def malformed(paired):
    """-> [(name, text, kind, 1-based line)]: for every rule a file whose only offender breaks it (and, where a line can, later
    rules too: the first in the order is reported), and a file `X_after` where that offender stands BEHIND an earlier line that
    breaks a later rule (FIELDS for the last one): the lowest line is reported, not the first rule."""
    F, N, G, R, C, Ln = 1, 2, 4, 8, 16, 32
    bad_flag = 99 | 0x80 if paired else 99                     # both mates / a paired flag in a single-end call
    raw = lambda q, flag, rname, pos, cigar, seq: b"\t".join([q, flag, rname, pos, b"255", cigar, b"*", b"0", b"0", seq, b"*"]) + b"\n"
    ok_flag = b"73" if paired else b"0"
    offender = {
        F: b"short\t%s\ttA\t1\t255\t50M\t*\t0\t0\t*\n" % ok_flag,                                  # ten fields
        N: raw(b"num", ok_flag, b"nowhere", b"0", b"5Q", b"*"),                                       # POS 0, and RNAME, CIGAR
        G: raw(b"flag", b"%d" % bad_flag, b"nowhere", b"1", b"M", b"*"),                              # and RNAME, CIGAR
        R: raw(b"rname", ok_flag, b"tA.", b"1", b"1234567890M", b"*"),                                # and CIGAR
        C: raw(b"cigar", ok_flag, b"tA", b"1", b"10M5", b"A" * 70000),                               # (the length is not looked at)
        Ln: raw(b"len", ok_flag, b"tA", b"1", b"10M", b"A" * 11),
    }
    names = {F: "fields", N: "number", G: "flag", R: "rname", C: "cigar", Ln: "length"}
    out = []
    for kind, text in offender.items():
        pre = header() + good_group(paired, b"g1") + good_group(paired, b"g2", 1)
        out.append((names[kind], pre + text + good_group(paired, b"g3"), kind, pre.count(b"\n") + 1))
        earlier_kind = F if kind == Ln else kind * 2
        earlier = offender[earlier_kind]
        out.append((names[kind] + "_after", pre + earlier + good_group(paired, b"g3") + text, earlier_kind, pre.count(b"\n") + 1))
    # more ways to break each rule, one per file
    more = [("empty_line", b"\n", F), ("cr_only", b"\r\n", F), ("flag_6_digits", raw(b"x", b"000073", b"tA", b"1", b"*", b"*"), N),
            ("flag_65536", raw(b"x", b"65536", b"tA", b"1", b"*", b"*"), N), ("flag_sign", raw(b"x", b"+73", b"tA", b"1", b"*", b"*"), N),
            ("flag_empty", raw(b"x", b"", b"tA", b"1", b"*", b"*"), N), ("pos_2_31", raw(b"x", ok_flag, b"tA", b"2147483648", b"*", b"*"), N),
            ("pos_11_digits", raw(b"x", ok_flag, b"tA", b"00000000001", b"*", b"*"), N),
            ("rname_star", raw(b"x", ok_flag, b"*", b"1", b"*", b"*"), R), ("rname_case", raw(b"x", ok_flag, b"Ta", b"1", b"*", b"*"), R),
            ("cigar_empty", raw(b"x", ok_flag, b"tA", b"1", b"", b"*"), C), ("cigar_no_count", raw(b"x", ok_flag, b"tA", b"1", b"M", b"*"), C),
            ("cigar_star_star", raw(b"x", ok_flag, b"tA", b"1", b"**", b"*"), C), ("cigar_lower", raw(b"x", ok_flag, b"tA", b"1", b"50m", b"*"), C),
            ("len_65536", raw(b"x", ok_flag, b"tA", b"1", b"65536M", b"*"), Ln), ("len_seq_empty", raw(b"x", ok_flag, b"tA", b"1", b"5M", b""), Ln)]
    if paired:
        more += [("flag_unpaired", raw(b"x", b"0", b"tA", b"1", b"*", b"*"), G), ("flag_no_mate_bit", raw(b"x", b"1", b"tA", b"1", b"*", b"*"), G),
                 ("flag_unmapped_unpaired", raw(b"x", b"4", b"*", b"0", b"*", b"*"), G)]
    for name, text, kind in more:
        pre = good_group(paired, b"g1")
        out.append((name, pre + text + good_group(paired, b"g3"), kind, 3))
    return out


def random_sam(seed, paired, n_fragments=300):
    """a few hundred fragments: every kind of group the rules tell apart, in random order and sizes"""
    rng = random.Random(seed)
    out = [header(b"\r\n" if seed % 2 else b"\n")]
    for f in range(n_fragments):
        q = b"frag%d" % rng.randrange(n_fragments // 3) if rng.random() < 0.3 else b"f%d.%d" % (seed, f)     # (neighbours may share a name)
        eol = b"\r\n" if rng.random() < 0.1 else b"\n"
        lines = []
        for _ in range(rng.choice([1, 1, 2, 2, 2, 3, 4, 7, 20])):
            t = rng.choice([0, 1, 2, 3, 4, 6])
            n = rng.randrange(20, 120)
            pos = rng.randrange(1, 700)
            clip = rng.randrange(0, 10)
            cigar = rng.choice([m50(n), b"%dS%dM" % (clip + 1, n - clip - 1), b"%dH%dM" % (clip + 1, n), b"*"])
            seq = b"ACGT"[rng.randrange(4):][:1] * n if cigar == b"*" or rng.random() < 0.3 else b"*"
            rev = 0x10 if rng.random() < 0.5 else 0
            sec = 0x100 if lines else 0
            kind = rng.random()
            if kind < 0.55:      # a pair, sometimes on two transcripts or in the wrong order
                t2 = t if rng.random() < 0.8 else rng.choice([0, 1, 2])
                a = line(paired, q, 0x41 | sec | rev, t, pos, cigar, seq, eol)
                b = line(paired, q, 0x81 | sec | (rev ^ 0x10), t2, pos + rng.randrange(0, 200), m50(n), eol=eol)
                lines += [b, a] if rng.random() < 0.1 else [a, b]
            elif kind < 0.8:
                lines.append(line(paired, q, (0x41 if rng.random() < 0.5 else 0x81) | 0x8 | sec | rev, t, pos, cigar, seq, eol))
            elif kind < 0.9:
                lines += [line(paired, q, 77, eol=eol), line(paired, q, 141, eol=eol)]
            else:
                lines.append(line(paired, q, 0x800 | 0x41 | rev, t, pos, cigar, seq, eol))
        out += lines
        if rng.random() < 0.02:
            out.append(b"@CO\tcomment %d\n" % f)
    text = b"".join(out)
    return text[:-1] if seed % 3 == 0 and text.endswith(b"\n") and not text.endswith(b"\r\n") else text
