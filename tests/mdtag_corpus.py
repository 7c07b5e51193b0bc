"""The batches the NM / MD tag tests share (tests/test_mdtag_cpu.py, tests/test_gpu_mdtag.py).  Hand-made mates on a few transcripts
of tens to a few thousand bases, each run paired, as both orphan kinds and single end, on both strands and with a secondary record:
no mismatch; a mismatch at the first and at the last M column; two adjacent mismatches; MD runs of 9 / 10 / 99 / 100 / 999 / 1000
matches; mates of 1, 15, 16, 17, 31, 32, 33, 255, 256 and 257 bases; pos < 0 (a left soft clip); an M run over the transcript's right
end; lower-case and non-letter transcript bytes; N in the read and in the transcript at the same column; mates with exactly 127 / 128
/ 255 / 256 mismatches; a mate of 3 000 bases that mismatches in every column; reads with 127 / 128 / 255 / 256 records; a batch of
only record-less reads; no reads at all.  With alignments: 50M2D50M, a deletion directly followed by a mismatch, 50M2I50M all
matching, clips at both ends, an unalignable slot, hand-made operations that use = and X and N -- and the gapped-alignment corpus
(tests/aligng_corpus.py) with the statement's own alignments at max_indel 3.  Built once a process; the statement is computed once a
case and shared."""
import functools
import struct

import numpy as np

import aligng_corpus as AG
import verify_corpus as VC
from oracle import oracle as O

SUB = bytes.maketrans(b"ACGTacgt", b"CGTAcgta")          # a base that differs, in the same case
LENGTHS = (1, 15, 16, 17, 31, 32, 33, 255, 256, 257)
RUNS = (9, 10, 99, 100, 999, 1000)
MISMATCHES = (127, 128, 255, 256)
NH_EDGES = (127, 128, 255, 256)


def _rec(tid, pos, st, fwd, mate_pos=0, mate_fwd=0, a=0, b=0):
    return (tid, pos, mate_pos if st == 3 else 0, 0, a & 0xFFFF, b & 0xFFFF, fwd, mate_fwd if st == 3 else 0, st, 0)


def _sub_at(m, *at):
    b = bytearray(m)
    for i in at:
        b[i] = b[i:i + 1].translate(SUB)[0]
    return bytes(b)


def _variants(seqs, items, kind):
    """items: (tid, pos, the mate as it lies on the transcript's strand).  kind "se": per item a forward and a reverse read, each
    with a secondary record three bases on; "pe": per item two pairs (mate 1 forward and mate 2 reverse, and the other way round),
    mate 2 being the next item's mate on the same transcript or the item's own, with a secondary record; "orphan": both orphan kinds
    on both strands"""
    r1, r2, recs, off = [], [], [], [0]
    for n, (tid, pos, m) in enumerate(items):
        tid2, pos2, m2 = items[(n + 1) % len(items)]
        if tid2 != tid:
            tid2, pos2, m2 = tid, pos, m
        for fwd in (1, 0):
            own = m if fwd else VC.revcomp(m)
            if kind == "se":
                r1.append(own)
                recs += [_rec(tid, pos, 0, fwd, a=len(m)), _rec(tid, pos + 3, 0, fwd, a=len(m))]
            elif kind == "pe":
                r1.append(own); r2.append(VC.revcomp(m2) if fwd else m2)
                recs += [_rec(tid, pos, 3, fwd, pos2, 1 - fwd, len(m), len(m2)), _rec(tid, pos2, 3, fwd, pos, 1 - fwd, len(m), len(m2))]
            else:
                r1.append(own); r2.append(VC.revcomp(m2) if fwd else m2)
                recs += [_rec(tid, pos, 1, fwd, a=len(m), b=len(m2)), _rec(tid, pos2, 2, 1 - fwd, a=len(m2), b=len(m))]
            off.append(len(recs))
    return VC._case(seqs, r1, r2 if kind != "se" else None, np.array(recs, dtype=O.HIT_DTYPE), off)


def _hand_items():
    rng = np.random.default_rng(21)
    t0 = bytes(rng.choice(VC.ACGT, 2600))
    odd = bytearray(rng.choice(VC.ACGT, 90))
    for i, ch in ((3, b"n"), (10, b"N"), (17, b"*"), (18, b"-"), (30, b"r"), (31, b"Y"), (44, b"."), (60, b"\x00"), (61, b"\xe9"), (62, b"@"), (63, b"[")):
        odd[i] = ch[0]
    odd = bytes(odd[:45]).lower() + bytes(odd[45:])
    t3 = bytes(rng.choice(VC.ACGT, 3100))
    seqs = [t0, odd, t3, t0[:40]]
    edges, runs, lens, special, heavy = [], [], [], [], []
    edges.append((0, 200, t0[200:270]))                                           # no mismatch
    edges.append((0, 300, _sub_at(t0[300:370], 0)))                               # the first M column
    edges.append((0, 400, _sub_at(t0[400:470], 69)))                              # the last
    edges.append((0, 500, _sub_at(t0[500:570], 0, 69)))
    edges.append((0, 600, _sub_at(t0[600:670], 30, 31)))                          # ..A0C..
    edges.append((0, 700, _sub_at(t0[700:770], 15, 16, 17, 47, 48)))              # across the lanes' edges
    edges.append((0, -5, bytes(rng.choice(VC.ACGT, 5)) + t0[:40]))                # pos < 0
    edges.append((0, -16, bytes(rng.choice(VC.ACGT, 16)) + _sub_at(t0[:33], 0, 32)))
    edges.append((0, len(t0) - 20, t0[-20:] + bytes(rng.choice(VC.ACGT, 10))))    # over the right end
    edges.append((3, 30, t0[30:40] + bytes(rng.choice(VC.ACGT, 30))))
    for run in RUNS:
        runs.append((0, 100, _sub_at(t0[100:100 + run + 2], 0, run + 1)))         # 0X<run>Y0
        runs.append((0, 150, _sub_at(t0[150:150 + run + 1], 0)))                  # 0X<run>
        runs.append((0, 170, _sub_at(t0[170:170 + run + 1], run)))                # <run>X0
    for n in LENGTHS:
        lens.append((0, 1000 + n, t0[1000 + n:1000 + 2 * n]))
        lens.append((0, 1300 + n, _sub_at(t0[1300 + n:1300 + 2 * n], n - 1)))
        lens.append((0, 1600 + n, _sub_at(t0[1600 + n:1600 + 2 * n], 0, n // 2)))
    up = odd.upper()
    special.append((1, 0, up[:90].replace(b"*", b"A").replace(b"-", b"C")))        # lower case matches; non-letters never do
    special.append((1, 5, _sub_at(up[5:80], 20, 40)))
    special.append((1, 2, up[2:9] + b"N" + up[10:50]))                            # N over N
    special.append((1, 0, up[:3] + b"N" + up[4:40]))                              # N over n
    special.append((0, 900, t0[900:920] + b"N" + t0[921:960]))                    # N in the read alone
    for k in MISMATCHES:
        heavy.append((0, 2000, _sub_at(t0[2000:2300], *range(k))))
        heavy.append((0, 2000, _sub_at(t0[2000:2300], *range(1, 2 * k, 2)) if 2 * k <= 300 else _sub_at(t0[2000:2300], *range(300 - k, 300))))
    heavy.append((2, 50, t3[50:3050].translate(SUB)))                             # 3 000 bases, every column a mismatch
    return seqs, dict(edges=edges, runs=runs, lens=lens, special=special, heavy=heavy)


def _many_records():
    """single-end reads of 20 bases with 127 / 128 / 255 / 256 records, and reads without one between them"""
    rng = np.random.default_rng(22)
    t = bytes(rng.choice(VC.ACGT, 400))
    r1, recs, off = [], [], [0]
    for k in NH_EDGES:
        r1.append(t[100:120])
        recs += [_rec(0, 100 - (i % 90) + (i // 90), 0, 1, a=20) for i in range(k)]
        off.append(len(recs))
        r1.append(t[:20]); off.append(len(recs))
    return VC._case([t], r1, None, np.array(recs, dtype=O.HIT_DTYPE), off)


def _with_alignments():
    """-> (case, (pos, nm, op_off, ops)): hand-made operations, single end, both strands; nm is the rule's own (filled by expected())"""
    rng = np.random.default_rng(23)
    t = bytes(rng.choice(VC.ACGT, 400))
    M, I, D, N, S, EQ, X = 0, 1, 2, 3, 4, 7, 8
    w = lambda n, op: n << 4 | op
    items = [
        (t[100:150] + t[152:202], 100, [w(50, M), w(2, D), w(50, M)]),
        (t[100:150] + _sub_at(t[152:202], 0), 100, [w(50, M), w(2, D), w(50, M)]),                    # ^AC0T
        (t[100:150] + bytes(rng.choice(VC.ACGT, 2)) + t[150:200], 100, [w(50, M), w(2, I), w(50, M)]),  # MD 100
        (bytes(rng.choice(VC.ACGT, 5)) + t[60:100] + bytes(rng.choice(VC.ACGT, 5)), 60, [w(5, S), w(40, M), w(5, S)]),
        (t[10:30], 0, []),                                                                            # unalignable
        (_sub_at(t[200:221], 10), 200, [w(10, EQ), w(1, X), w(10, EQ)]),
        (t[200:221], 200, [w(10, EQ), w(1, X), w(10, EQ)]),                                           # (an X that matches: the rule compares)
        (t[250:260] + t[300:320], 250, [w(10, M), w(40, N), w(20, M)]),
        (t[0:30] + t[31:300], 0, [w(30, M), w(1, D), w(269, M)]),                                     # 269 M columns: two steps of a group
        (t[380:400] + t[0:10], 380, [w(20, M), w(10, S)]),
        (t[20:40], 20, [w(3, 5), w(20, M), w(2, 6)]),                                                 # H and P move nothing
    ]
    r1, recs, off, pos, n_ops, ops = [], [], [0], [], [], []
    for m, x0, words in items:
        for fwd in (1, 0):
            r1.append(m if fwd else VC.revcomp(m))
            recs.append(_rec(0, x0, 0, fwd, a=len(m)))
            off.append(len(recs))
            pos += [x0 if words else 0, 0]; n_ops += [len(words), 0]; ops += words
    case = VC._case([t], r1, None, np.array(recs, dtype=O.HIT_DTYPE), off)
    aln = (np.array(pos, np.int32), np.zeros(len(pos), np.uint32), np.concatenate([[0], np.cumsum(n_ops)]).astype(np.uint64), np.array(ops, np.uint32))
    return case, aln


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (case, alignment or None)"""
    seqs, items = _hand_items()
    out = {}
    for group, its in items.items():
        for kind in ("se", "pe", "orphan"):
            out["%s_%s" % (group, kind)] = (_variants(seqs, its, kind), None)
    out["many_records"] = (_many_records(), None)
    out["hand_ops"] = _with_alignments()
    t = seqs[0]
    none = np.zeros(0, dtype=O.HIT_DTYPE)
    out["no_records_pe"] = (VC._case(seqs, [t[:30], t[40:75], b""], [t[100:130], b"A", t[5:9]], none, [0, 0, 0, 0]), None)
    out["no_records_se"] = (VC._case(seqs, [t[:30], t[40:75]], None, none, [0, 0, 0]), None)
    out["no_reads"] = (VC._case(seqs, [], None, none, [0]), None)
    for name in ("pe_indel", "se_indel", "edges_pe", "edges_se", "indels_pe", "homopolymers", "long"):
        c = AG.cases()[name]
        out["ag_" + name] = (c, None)
        out["ag_" + name + "_aligned"] = (c, AG.expected(name, 3)[:4])
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """md_tags_host of a case: (nm, md_off, md, stats), computed once, shared, never changed"""
    from sailfish_amd import hits as H
    c, aln = cases()[name]
    out = H.md_tags_host(c["seqs"], c["hits"], c["off"], c["r1"], c["r2"], aln)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def md_strings(name):
    """the MD of every slot as bytes"""
    _, md_off, md, _ = expected(name)
    raw = md.tobytes()
    return [raw[int(a):int(b)] for a, b in zip(md_off[:-1], md_off[1:])]


def slot_lines(case, aln):
    """what the writer says of every slot that is a line: slot -> (read, mate bytes as sequenced, forward?, tid, POS - 1, CIGAR words)"""
    from sailfish_amd import hits as H
    out = {}
    for r in range(len(case["off"]) - 1):
        for i in range(case["off"][r], case["off"][r + 1]):
            h = case["hits"][i]
            for j, (rd, fwd, _) in enumerate(H._record_jobs(h, r, case["r1"], case["r2"])):
                s = 2 * i + j
                if aln is not None:
                    words, x = [int(w) for w in aln[3][int(aln[2][s]):int(aln[2][s + 1])]], int(aln[0][s])
                else:
                    pos, n = (int(h["mate_pos"]), int(h["mate_len"])) if j else (int(h["pos"]), int(h["read_len"]))
                    words, x = ([n << 4], pos) if pos >= 0 else ([-pos << 4 | 4, (n + pos) << 4], 0) if -pos < n else ([], 0)
                out[s] = (r, rd, fwd, int(h["tid"]), x, words)
    return out


def blob(name):
    """a case with its expected result as the byte string tests/mdtag_harness.cpp's stand-alone program reads"""
    from sailfish_amd import hits as H
    c, aln = cases()[name]
    nm, md_off, md, st = expected(name)
    ts, toff = VC.packed(c["seqs"])
    s1, o1 = VC.packed(c["r1"])
    s2, o2 = VC.packed(c["r2"]) if c["r2"] is not None else (np.zeros(0, np.uint8), np.zeros(0, np.uint64))
    tl = np.array([len(x) for x in c["seqs"]], np.uint32)
    n_words = len(aln[3]) if aln is not None else 0
    head = struct.pack("<10Q", len(c["seqs"]), len(ts), len(c["r1"]), len(s1), len(s2), len(c["hits"]), int(c["r2"] is not None), int(aln is not None),
                       n_words, len(md))
    stats = np.array([st[key] for key in H.MDTAG_STATS], np.uint64)
    parts = [ts, toff[:-1], tl, s1, o1, s2, o2, c["hits"], c["off"]]
    if aln is not None:
        parts += [aln[0].astype(np.int32), aln[2].astype(np.uint64), aln[3].astype(np.uint32)]
    parts += [nm, md_off, md, stats]
    return head + b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


# ---- what the writers are given ---------------------------------------------------------------------------------------------------

WRITABLE = ("edges_se", "edges_pe", "edges_orphan", "runs_se", "runs_pe", "lens_se", "lens_pe", "lens_orphan", "special_se", "special_pe", "heavy_se", "heavy_pe",
            "heavy_orphan", "many_records", "hand_ops", "no_records_pe", "no_records_se", "ag_pe_indel_aligned", "ag_se_indel_aligned", "ag_homopolymers_aligned",
            "ag_long_aligned")


@functools.lru_cache(maxsize=None)
def writable(name):
    """a case without the records that hold a slot without an operation (SAM cannot say them) -> (case, alignment or None, tags):
    the arrays are the statement's own, cut"""
    c, aln = cases()[name]
    nm, md_off, md, _ = expected(name)
    if aln is None:
        return c, None, (nm, md_off, md)
    n_ops = np.diff(aln[2].astype(np.int64))
    keep = np.array([all(n_ops[2 * i + j] > 0 for j in range(2 if c["hits"][i]["mate_status"] == 3 else 1)) for i in range(len(c["hits"]))], bool)
    off = np.concatenate([[0], np.cumsum([int(keep[c["off"][r]:c["off"][r + 1]].sum()) for r in range(len(c["off"]) - 1)])]).astype(np.uint32)
    slots = np.nonzero(np.repeat(keep, 2))[0]
    cut = lambda o, v: ([v[int(o[s]):int(o[s + 1])] for s in slots])
    words, texts = cut(aln[2], aln[3]), cut(md_off, md)
    csr = lambda parts: np.concatenate([[0], np.cumsum([len(w) for w in parts])]).astype(np.uint64)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return (VC._case(c["seqs"], c["r1"], c["r2"], c["hits"][keep], off), (aln[0][slots].copy(), aln[1][slots].copy(), csr(words), cat(words, np.uint32)),
            (nm[slots].copy(), csr(texts), cat(texts, np.uint8)))


def qnames_case(first_name_len):
    """120 single-end reads of 20 bases, a mismatch each, on both strands; read 0 is named x * first_name_len, so that every later line
    -- and with it the 4 096-byte tile edges -- moves a byte a step through the lines' tag fields -> (case, read names)"""
    rng = np.random.default_rng(24)
    t = bytes(rng.choice(VC.ACGT, 300))
    r1, recs = [], []
    for i in range(120):
        m = _sub_at(t[i:i + 20], i % 20)
        r1.append(m if i % 2 else VC.revcomp(m))
        recs.append(_rec(0, i, 0, i % 2, a=20))
    names = [b"x" * first_name_len] + [b"q%d" % i for i in range(1, 120)]
    return VC._case([t], r1, None, np.array(recs, dtype=O.HIT_DTYPE), list(range(121))), names
