"""The batches the gapped-alignment tests share (tests/test_aligng_cpu.py, tests/test_gpu_aligng.py), built from the gapped
verification corpus's makers (tests/verifyg_corpus.py): mapped reads with substitutions and indels, reduced to the records that
verify_hits_gapped_host keeps at 0.9 and max_indel 3 (pairs and single end); the hand-made records of every mate status, kept whole
as the survivors of permille 0 -- both orphan kinds, both strands, pos < 0, overhang at the right end, records wholly off their
transcript (unalignable jobs), N, lower case, mates of 0, 1, 2, 15, 16, 17, 31, 32, 33, 100 and 257 bases; indels of exactly k and
k + 1 bases for every k of the grid; the issue's first thing to look at (two transcript bases deleted in the middle of a mate of 100,
recorded in front of and behind the gap); gaps in homopolymer runs, where the tie rules decide; and one mate of 2 000 bases with
three indels, on either strand; and 512 short records, a record count at which the device's per-slot arrays fill their blocks
exactly.  Built once a process; the statement is computed once per (case, k) and shared."""
import functools
import struct

import numpy as np

import verify_corpus as VC
import verifyg_corpus as VG
from oracle import oracle as O

KS = VG.KS


def _survivors(case, permille, k):
    from sailfish_amd import hits as H
    h, o, _, _ = H.verify_hits_gapped_host(case["seqs"], case["hits"], case["off"], case["r1"], case["r2"], permille, False, k)
    return VC._case(case["seqs"], case["r1"], case["r2"], h, o)


def first_look():
    """t[100:150] + t[152:202] on one transcript, recorded once at pos 100 and once at pos 102 (the seed behind the gap)"""
    rng = np.random.default_rng(5)
    t = bytes(rng.choice(VC.ACGT, 400))
    read = t[100:150] + t[152:202]
    recs = [VG._rec(0, 100, 0, 1, a=100), VG._rec(0, 102, 0, 1, a=100)]
    return VC._case([t], [read, read], None, np.array(recs, dtype=O.HIT_DTYPE), [0, 1, 2])


def homopolymers():
    """a deletion and an insertion of 1 - 3 bases inside runs of one base, on either strand, recorded on either side of the gap: many
    optimal paths tie, the rule picks one"""
    rng = np.random.default_rng(9)
    t = b"".join(bytes([int(rng.choice(VC.ACGT))]) * int(rng.integers(1, 9)) for _ in range(120))
    r1, recs, off = [], [], [0]
    for _ in range(40):
        a = int(rng.integers(0, len(t) - 90))
        n = int(rng.integers(1, 4))
        p = int(rng.integers(10, 60))
        m = t[a:a + p] + (t[a + p + n:a + 80 + n] if rng.random() < 0.5 else bytes([t[a + p]]) * n + t[a + p:a + 80 - n])
        fwd = rng.random() < 0.5
        r1.append(m if fwd else VC.revcomp(m))
        recs.append(VG._rec(0, a + int(rng.integers(-n, n + 1)), 0, int(fwd), a=len(m)))
        off.append(len(recs))
    return VC._case([t], r1, None, np.array(recs, dtype=O.HIT_DTYPE), off)


def long_mate():
    """one mate of 2 000 bases with 1 % substitutions, 2 bases deleted at 300, 3 inserted at 900 and 1 deleted at 1 500, forward and as
    its reverse complement, hanging 40 bases over the transcript's right end"""
    rng = np.random.default_rng(6)
    t = bytes(rng.choice(VC.ACGT, 2100))
    m = VC.with_errors(rng, [t[140:2100] + bytes(rng.choice(VC.ACGT, 60))], 0.01)[0]
    m = (m[:300] + m[302:900] + b"GAT" + m[900:1500] + m[1501:])[:2000]
    recs = [VG._rec(0, 140, 0, 1, a=2000), VG._rec(0, 140, 0, 0, a=2000)]
    return VC._case([t, t[:50]], [m, VC.revcomp(m)], None, np.array(recs, dtype=O.HIT_DTYPE), [0, 1, 2])


def power_of_two():
    """512 records, 1 024 slots: the per-slot scratch arrays fill whole power-of-two blocks to the last byte, 4 096 of them here, so
    a pass that reads one entry too many leaves its block.  Mates of 20 - 28 bases, a third exact, a third with a substitution, a
    third with a base deleted"""
    rng = np.random.default_rng(8)
    t = bytes(rng.choice(VC.ACGT, 700))
    r1, recs = [], []
    for i in range(512):
        a, n = int(rng.integers(0, 660)), int(rng.integers(20, 29))
        m = bytearray(t[a:a + n + 1])
        if i % 3 == 1:
            m[n // 2] = {65: 67, 67: 71, 71: 84, 84: 65}[m[n // 2]]
        m = bytes(m[:n // 2] + m[n // 2 + 1:]) if i % 3 == 2 else bytes(m[:n])
        fwd = i % 2
        r1.append(m if fwd else VC.revcomp(m))
        recs.append(VG._rec(0, a, 0, fwd, a=n))
    return VC._case([t], r1, None, np.array(recs, dtype=O.HIT_DTYPE), list(range(513)))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case (seqs, r1, r2 or None, hits, off)"""
    return {
        "pe_indel": _survivors(VG._mapped(71, 110, 70, True), 900, 3),
        "se_indel": _survivors(VG._mapped(72, 140, 70, False), 900, 3),
        "edges_pe": VG._edges(61, True),
        "edges_se": VG._edges(62, False),
        "indels_pe": _survivors(VG._indels(True), 0, 3),
        "indels_se": _survivors(VG._indels(False), 0, 3),
        "first_look": first_look(),
        "homopolymers": homopolymers(),
        "long": long_mate(),
        "power_of_two": power_of_two(),
    }


@functools.lru_cache(maxsize=None)
def expected(name, k):
    """align_hits_host of a case: (pos, nm, op_off, ops, stats, detail), computed once per (case, k), shared, never changed"""
    from sailfish_amd import hits as H
    c = cases()[name]
    out = H.align_hits_host(c["seqs"], c["hits"], c["off"], c["r1"], c["r2"], k)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def lengths(case):
    """the mate's length of every slot, -1 where the slot is no job"""
    n = len(case["hits"])
    out = np.full(2 * n, -1, np.int64)
    for r in range(len(case["off"]) - 1):
        for i in range(case["off"][r], case["off"][r + 1]):
            st = int(case["hits"][i]["mate_status"])
            out[2 * i] = len(case["r2"][r] if st == 2 else case["r1"][r])
            if st == 3:
                out[2 * i + 1] = len(case["r2"][r])
    return out


def blob(name, k):
    """a case with its expected result as the byte string tests/aligng_harness.cpp's stand-alone program reads"""
    from sailfish_amd import hits as H
    c = cases()[name]
    pos, nm, op_off, ops, st, detail = expected(name, k)
    ts, toff = VC.packed(c["seqs"])
    s1, o1 = VC.packed(c["r1"])
    s2, o2 = VC.packed(c["r2"]) if c["r2"] is not None else (np.zeros(0, np.uint8), np.zeros(0, np.uint64))
    tl = np.array([len(x) for x in c["seqs"]], np.uint32)
    head = struct.pack("<9Q", len(c["seqs"]), len(ts), len(c["r1"]), len(s1), len(s2), len(c["hits"]), int(c["r2"] is not None), len(ops), k)
    stats = np.array([st[key] for key in H.ALIGNG_STATS], np.uint64)
    parts = [ts, toff[:-1], tl, s1, o1, s2, o2, c["hits"], c["off"], pos, nm, op_off, ops, detail.astype(np.uint64), stats]
    return head + b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def replay(case, name_k_result):
    """every slot's operations replayed over the mate's oriented bases and the transcript from pos -> (nm, read bases consumed,
    reference span) per slot, -1 where the slot has no operations; an aligned base off the transcript is an AssertionError"""
    from sailfish_amd import hits as H
    pos, nm, op_off, ops = name_k_result[:4]
    n = len(case["hits"])
    out = np.full((2 * n, 3), -1, np.int64)
    for r in range(len(case["off"]) - 1):
        for i in range(case["off"][r], case["off"][r + 1]):
            t = H._BASE_CODE[np.frombuffer(case["seqs"][int(case["hits"][i]["tid"])], np.uint8)]
            for j, (rd, fwd, _) in enumerate(H._record_jobs(case["hits"][i], r, case["r1"], case["r2"])):
                s = 2 * i + j
                words = [int(w) for w in ops[int(op_off[s]):int(op_off[s + 1])]]
                if not words:
                    continue
                c = H._BASE_CODE[np.frombuffer(rd, np.uint8)]
                a = c if fwd else np.where(c > 3, 4, 3 - c).astype(np.uint8)[::-1]
                q, x, got = 0, int(pos[s]), 0
                for w in words:
                    ln, op = w >> 4, w & 15
                    assert ln > 0 and op in (H.CIGAR_M, H.CIGAR_I, H.CIGAR_D, H.CIGAR_S), (s, words)
                    if op == H.CIGAR_M:
                        assert 0 <= x and x + ln <= len(t), (s, words, x)
                        aa, bb = a[q:q + ln], t[x:x + ln]
                        got += int(((aa > 3) | (aa != bb)).sum())
                        q += ln; x += ln
                    elif op == H.CIGAR_D:
                        got += ln; x += ln
                    else:
                        got += ln if op == H.CIGAR_I else 0
                        q += ln
                out[s] = (got, q, x - int(pos[s]))
    return out


@functools.lru_cache(maxsize=None)
def writable(name, k):
    """a case without the records that hold an unalignable job (SAM cannot say them), with the statement's alignment of what is left
    -> (case, (pos, nm, op_off, ops)); the arrays are the statement's own, cut"""
    c = cases()[name]
    pos, nm, op_off, ops = expected(name, k)[:4]
    n_ops = np.diff(op_off.astype(np.int64))
    keep = np.array([all(n_ops[2 * i + j] > 0 for j in range(2 if c["hits"][i]["mate_status"] == 3 else 1)) for i in range(len(c["hits"]))], bool)
    off = np.concatenate([[0], np.cumsum([int(keep[c["off"][r]:c["off"][r + 1]].sum()) for r in range(len(c["off"]) - 1)])]).astype(np.uint32)
    slots = np.repeat(keep, 2)
    words = [ops[int(op_off[s]):int(op_off[s + 1])] for s in np.nonzero(slots)[0]]
    new_off = np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.uint64)
    new_ops = np.concatenate(words).astype(np.uint32) if words else np.zeros(0, np.uint32)
    return VC._case(c["seqs"], c["r1"], c["r2"], c["hits"][keep], off), (pos[slots].copy(), nm[slots].copy(), new_off, new_ops)


def sam_inputs(case):
    """what samfile._sam_text takes for a case: (names, ref_len, seqs per read)"""
    names = [b"t%d" % i for i in range(len(case["seqs"]))]
    seqs = list(case["r1"]) if case["r2"] is None else list(zip(case["r1"], case["r2"]))
    return names, np.array([len(s) for s in case["seqs"]], np.uint32), seqs


def is_paired(case):
    """as samfile._sam_text decides it"""
    return bool((case["hits"]["mate_status"] != 0).any()) if len(case["hits"]) else case["r2"] is not None
