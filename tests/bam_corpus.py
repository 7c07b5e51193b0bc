"""BAM streams (inflated: what lies behind the BGZF layer) shared by test_bam_cpu.py (bamfmt.h serially, no GPU) and test_gpu_bam.py
(the device reader).  The well-formed SAM corpora of sam_corpus.py come through samfile.sam_to_bam; what that converter cannot
write is built here from raw fields: one stream per broken rule, a decoy stream whose tags hold fake records, and a spans stream
that is several supertiles of the device's chain resolution long.  Every generator takes `paired`, as in sam_corpus."""
import random
import struct

import sam_corpus

NAMES, REF_LEN, PAIR_BITS = sam_corpus.NAMES, sam_corpus.REF_LEN, sam_corpus.PAIR_BITS
EXTRA_REF = b"not_a_transcript"                          # a reference of the header that is no name of the run: refID len(NAMES)
TILE, SUPER = 4096, 64 * 4096                            # the production tile and supertile of csrc/bamtext.hip, in bytes
M, I, D, N, S, H, P, EQ, X = range(9)                    # CIGAR op codes


def header(refs=None, lens=None, text=b"@HD\tVN:1.6\tSO:unsorted\n"):
    refs = NAMES + [EXTRA_REF] if refs is None else refs
    lens = REF_LEN + [100] if lens is None else lens
    return b"".join([b"BAM\x01", struct.pack("<I", len(text)), text, struct.pack("<I", len(refs))] +
                    [struct.pack("<I", len(n) + 1) + n + b"\0" + struct.pack("<I", l) for n, l in zip(refs, lens)])


def record(paired, q, flag, ref=-1, pos=-1, cigar=(), l_seq=0, tags=b"", *, block_size=None, l_read_name=None, name=None, words=None,
           n_cigar_op=None, seq_bytes=None):
    """one record from raw fields: every length field can be set apart from what follows it.  cigar: [(length, op)]; words: the
    CIGAR words as they stand; name: the name bytes as they stand (default q + NUL); seq_bytes: SEQ and QUAL as they stand."""
    if not paired:
        flag &= ~PAIR_BITS
    name = q + b"\0" if name is None else name
    words = [n << 4 | op for n, op in cigar] if words is None else words
    seq = bytes((l_seq + 1) // 2) + b"\xff" * l_seq if seq_bytes is None else seq_bytes
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name) if l_read_name is None else l_read_name, 255, 4680,
                       len(words) if n_cigar_op is None else n_cigar_op, flag, l_seq, -1, -1, 0)
    body += name + struct.pack("<%dI" % len(words), *words) + seq + tags
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def good_group(paired, q, t=0, pos=10):
    return record(paired, q, 99, t, pos, [(50, M)]) + record(paired, q, 147, t, pos + 100, [(50, M)])


def malformed(paired):
    """-> [(name, stream, kind, 1-based record)]: per rule a stream whose only offender breaks it (and later rules too, where a
    record can), its `_after` form (the offender stands BEHIND an earlier record that breaks a later rule: the lowest record is
    reported, not the first rule), and more ways to break each rule, one per stream.  The streams are final."""
    F, Nn, G, R, C, Ln = 1, 2, 4, 8, 16, 32
    ok = 73
    bad_flag = 99 | 0x80 if paired else 99
    n_ref = len(NAMES) + 1
    rec = lambda *a, **k: record(paired, *a, **k)
    whole = rec(b"short", ok, 0, 1, [(50, M)], tags=b"NHC\x01")
    offender = {
        F: rec(b"nonul", ok, 0, 1, [(50, M)], name=b"nonul!"),                                       # (the chain stays whole)
        Nn: rec(b"num", ok, -1, -1, words=[9]),                                                       # and RNAME, CIGAR
        G: record(True, b"flag", bad_flag, -1, 1, words=[9]),                                                 # and RNAME, CIGAR
        R: rec(b"rname", ok, n_ref, 1, words=[50 << 4 | 9]),                                          # and CIGAR
        C: rec(b"cigar", ok, 0, 1, words=[10 << 4 | M, 5 << 4 | 9], l_seq=70000),                    # (the length is not looked at)
        Ln: rec(b"len", ok, 0, 1, [(10, M)], l_seq=11),
    }
    names = {F: "fields", Nn: "number", G: "flag", R: "rname", C: "cigar", Ln: "length"}
    pre = header() + good_group(paired, b"g1") + good_group(paired, b"g2", 1)
    out = []
    for kind, text in offender.items():
        out.append((names[kind], pre + text + good_group(paired, b"g3"), kind, 5))
        earlier_kind = F if kind == Ln else kind * 2
        out.append((names[kind] + "_after", pre + offender[earlier_kind] + good_group(paired, b"g3") + text, earlier_kind, 5))
    more = [("block_size_31", rec(b"x", ok, 0, 1, block_size=31), F),
            ("block_size_negative", rec(b"x", ok, 0, 1, [(50, M)], block_size=-40), F),
            ("block_size_one_short", struct.pack("<i", len(whole) - 4 - 4 - 1) + whole[4:], F),
            ("l_read_name_0", rec(b"", ok, 0, 1, [(50, M)], name=b"", l_read_name=0), F),
            ("name_without_nul", offender[F], F),
            ("pos_minus_1", rec(b"x", ok, 0, -1, [(50, M)]), Nn), ("pos_2_31_minus_1", rec(b"x", ok, 0, 2 ** 31 - 1, [(50, M)]), Nn),
            ("ref_minus_1", rec(b"x", ok, -1, 1, [(50, M)]), R), ("ref_n_ref", rec(b"x", ok, n_ref, 1, [(50, M)]), R),
            ("ref_not_a_name", rec(b"x", ok, n_ref - 1, 1, [(50, M)]), R),
            ("op_code_9", rec(b"x", ok, 0, 1, words=[50 << 4 | 9]), C), ("op_code_15", rec(b"x", ok, 0, 1, words=[10 << 4 | M, 15]), C),
            ("l_seq_65536", rec(b"x", ok, 0, 1, l_seq=65536), Ln), ("l_seq_not_qlen", rec(b"x", ok, 0, 1, [(5, S), (10, M), (3, D)], l_seq=14), Ln),
            ("qlen_65536", rec(b"x", ok, 0, 1, [(65536, M)]), Ln)]
    if paired:
        more += [("flag_unpaired", record(True, b"x", 0, 0, 1, [(50, M)]), G), ("flag_no_mate_bit", record(True, b"x", 1, 0, 1, [(50, M)]), G),
                 ("flag_unmapped_unpaired", record(True, b"x", 4), G)]
    for name, text, kind in more:
        out.append((name, pre + text + good_group(paired, b"g3"), kind, 5))
    g3 = good_group(paired, b"g3")
    out.append(("cut_inside_a_record", pre + g3[:len(g3) // 2 + 20], F, 6))
    out.append(("cut_inside_a_block_size", pre + g3 + g3[:2], F, 7))
    return out


def decoy(paired, n_groups=120):
    """Every record's tags hold three complete fake records: a valid block_size, refID, flag and NUL-terminated name each, chained
    to each other, at offsets that are no positions of the real chain (a short run of tag bytes stands in front).  Whoever looks
    for "what looks like a record" finds them; the chain does not.  -> the stream"""
    rng = random.Random(17)
    out = [header()]
    for g in range(n_groups):
        q = b"d%d" % g
        for flag, pos in ((99, 10 + g), (147, 150 + g)):
            fakes = b"".join(record(paired, b"fake%d" % k, 99 if k % 2 == 0 else 147, (g + 1 + k) % 5, 500 + k, [(30, M)]) for k in range(3))
            lead = b"XZZ"[: 1 + g % 3]                   # (the fakes at every alignment)
            trail = bytes(rng.randrange(1, 256) for _ in range(g % 4))
            out.append(record(paired, q, flag, g % 5, pos, [(50, M)], tags=lead + fakes + trail))
    return b"".join(out)


_SPANS = {}


def spans(paired):
    """About five supertiles of records: lengths from 44 to 400 bytes drawn until a record starts on every residue of the tile
    size (and so of 16), one record longer than a tile and one longer than a supertile (padded by a Z tag), and at the end one
    group of 5 000 records.  -> the stream"""
    if paired in _SPANS:
        return _SPANS[paired]
    rng = random.Random(5)
    out = [header()]
    at = len(out[0])
    missing = set(range(TILE))
    k = 0

    def add(r):
        nonlocal at
        missing.discard(at % TILE)
        out.append(r)
        at += len(r)

    while missing:
        q = b"s%d" % (k // 2)
        base = record(paired, q, 147 if k % 2 else 99, k // 2 % 5, 1 + k % 700, [(40, M)])
        want = [n for n in range(max(44, len(base)), 401) if (at + n) % TILE in missing]
        n = rng.choice(want) if want and rng.random() < 0.9 else rng.randrange(max(44, len(base)), 401)
        add(struct.pack("<i", n - 4) + base[4:] + bytes(rng.randrange(256) for _ in range(n - len(base))))
        k += 1
        if k == 1500:
            add(record(paired, b"tile", 73, 6, 5, [(40, M)], tags=b"XZZ" + b"t" * (TILE + 900) + b"\0"))
        if k == 2500:
            add(record(paired, b"super", 73, 6, 6, [(40, M)], tags=b"XZZ" + b"s" * (SUPER + 12345) + b"\0"))
    for i in range(2500):
        t = 6 - i % 7 if i % 7 != 1 else 6
        add(record(paired, b"big", 99 | (0x100 if i else 0), t, 1 + i, [(50, M)]))
        add(record(paired, b"big", 147 | (0x100 if i else 0), t, 101 + i, [(50, M)]))
    _SPANS[paired] = b"".join(out)
    return _SPANS[paired]
