"""The NM / MD tags without a GPU: csrc/mdfmt.h alone (tests/mdtag_harness.cpp, g++ -Wall -Wextra -Werror; once more as a
stand-alone program under -fsanitize=address,undefined) against the Python statement hits.md_tags_host over the shared corpus
(tests/mdtag_corpus.py); a few MDs worked by hand; and an independent judge written from the SAM specification, not from the rule:
rebuilding the reference from (SEQ, CIGAR, MD) of every oriented line gives the transcript's upper-cased bytes at POS, and NM is the
mismatches so rebuilt plus the I and D bases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aligng_corpus as AG
import mdtag_corpus as corpus
import verify_corpus as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "mdtag_harness.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
MD_RE = re.compile(rb"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*")
_P = C.c_void_p


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("mdh")), "libmdtag_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.mdh_tags.restype = C.c_int64
    L.mdh_tags.argtypes = [_P, _P, _P, C.c_uint64, _P, _P, _P, _P, C.c_uint32, _P, _P, _P, _P, _P, C.c_uint32, _P, _P, _P, C.c_uint64, _P]
    return L


def _one(t, read, pos, fwd=1, words=None, length=None):
    """(nm, MD) of one single-end record"""
    from sailfish_amd import hits as H
    rec = np.array([(0, pos, 0, 0, len(read) if length is None else length, 0, fwd, 0, 0, 0)], dtype=H.HIT_DTYPE)
    aln = None if words is None else (np.array([pos, 0], np.int32), None, np.array([0, len(words), len(words)], np.uint64), np.array(words, np.uint32))
    nm, md_off, md, st = H.md_tags_host([t], rec, [0, 1], [read], None, aln)
    assert md_off.tolist() == [0, len(md), len(md)] and nm[1] == 0 and st["slots"] == 1 and st["md_bytes"] == st["max_md_bytes"] == len(md)
    return int(nm[0]), md.tobytes(), st


def test_mds_worked_by_hand(built):
    """the issue's rule on lines small enough to read"""
    from sailfish_amd import hits as H
    assert H.MDTAG_STATS == ("slots", "sum_nm", "md_bytes", "max_md_bytes", "slots_plain")
    t = b"ACGTACGTAGCTAGCTAGGATCCATTGACCAGTTAGGCAT"
    assert _one(t, t[4:14], 4)[:2] == (0, b"10") and _one(t, t[4:14], 4)[2]["slots_plain"] == 1
    assert _one(t, VC.revcomp(t[4:14]), 4, fwd=0)[:2] == (0, b"10")
    assert _one(t, b"C" + t[5:14], 4)[:2] == (1, b"0A9")
    assert _one(t, t[4:13] + b"A", 4)[:2] == (1, b"9G0")
    assert _one(t, t[4:8] + b"CA" + t[10:14], 4)[:2] == (2, b"4A0G4")                                  # adjacent mismatches
    assert _one(t, VC.revcomp(t[4:8] + b"CA" + t[10:14]), 4, fwd=0)[:2] == (2, b"4A0G4")
    assert _one(t, b"GG" + t[:8], -2)[:2] == (0, b"8") and _one(t, b"GG" + t[:8], -2)[2]["slots_plain"] == 0      # 2S8M
    assert _one(t, t[36:] + b"AC", 36)[:2] == (2, b"4N0N0")                                              # over the right end
    assert _one(t, b"ACNT", 0)[:2] == (1, b"2G1")                                                        # N matches nothing
    assert _one(b"ACnTAC*Tac", b"ACNTACGTAC", 0)[:2] == (2, b"2N3N3")                                    # ... not even N; lower case matches
    assert _one(b"ACrTAC", b"ACATAC", 0)[:2] == (1, b"2R3")
    assert _one(t, t[:4], -4)[:2] == (0, b"0") and _one(t, t[:4], -9)[:2] == (0, b"0")                   # no base on the transcript
    assert _one(t, t[:4], 0, length=6)[:2] == (2, b"4A0C0")                                              # columns past the mate's bases
    M, I, D, S = H.CIGAR_M, H.CIGAR_I, H.CIGAR_D, H.CIGAR_S
    w = lambda n, op: n << 4 | op
    assert _one(t, t[4:8] + t[10:14], 4, words=[w(4, M), w(2, D), w(4, M)])[:2] == (2, b"4^AG4")
    assert _one(t, t[4:8] + b"A" + t[11:14], 4, words=[w(4, M), w(2, D), w(4, M)])[:2] == (3, b"4^AG0C3")  # a mismatch behind a deletion
    assert _one(t, t[4:8] + b"TT" + t[8:12], 4, words=[w(4, M), w(2, I), w(4, M)])[:2] == (2, b"8")
    assert _one(t, b"GG" + t[4:8] + b"GGG", 4, words=[w(2, S), w(4, M), w(3, S)])[:2] == (0, b"4")
    assert _one(t, t[4:8], 0, words=[])[:2] == (0, b"0")
    assert _one(t, t[4:7] + b"A", 4, words=[w(3, 7), w(1, 8)])[:2] == (1, b"3T0")
    bad = np.array([(0, 0, 0, 0, 4, 0, 1, 0, 0, 0), (3, 0, 0, 0, 4, 0, 1, 0, 0, 0)], dtype=H.HIT_DTYPE)
    with pytest.raises(ValueError, match="record 1 "):
        H.md_tags_host([t], bad, [0, 2], [b"ACGT"], None)
    with pytest.raises(ValueError, match="slots"):
        H.md_tags_host([t], bad[:1], [0, 1], [b"ACGT"], None, (np.zeros(4, np.int32), None, np.zeros(5, np.uint64), np.zeros(0, np.uint32)))


def _rebuild(seq, words, md):
    """the SAM specification's reading of (SEQ, CIGAR, MD) -> (the reference over the M and D columns, mismatches + I + D bases)"""
    tokens = re.findall(rb"[0-9]+|\^[A-Z]+|[A-Z]", md)
    assert b"".join(tokens) == md
    cols = []                                                                          # per reference column: None = SEQ's base, else the letter
    for tok in tokens:
        if tok.isdigit():
            cols += [None] * int(tok)
        elif tok.startswith(b"^"):
            cols += [(True, c) for c in tok[1:]]
        else:
            cols.append((False, tok[0]))
    ref, q, at, nm = bytearray(), 0, 0, 0
    for w in words:
        n, op = w >> 4, w & 15
        if op in (0, 7, 8):
            for _ in range(n):
                c = cols[at]; at += 1
                assert c is None or not c[0], "a deletion inside an M run"
                if c is None:
                    ref.append(seq[q:q + 1].upper()[0])
                else:
                    ref.append(c[1]); nm += 1
                q += 1
        elif op in (2, 3):
            for _ in range(n):
                c = cols[at]; at += 1
                assert c is not None and c[0], "an M column inside a deletion"
                ref.append(c[1])
            nm += n
        elif op in (1, 4):
            q += n
            nm += n if op == 1 else 0
    assert at == len(cols)
    return bytes(ref), nm, q


def test_the_statement_under_an_independent_judge(built):
    """every MD matches the specification's pattern; (SEQ, CIGAR, MD) of every oriented line rebuilds the transcript's upper-cased
    bytes at POS (N off the transcript and for what is no letter); NM is the rebuilt mismatches plus I and D; a missing slot is
    empty; the stats are the sums; and the corpus holds what the issue lists"""
    seen = dict(slots=0, runs=set(), lens=set(), nms=set(), caret0=0, clip=0, over=0, max_md=0, plain=0, statuses=set(), strands=set(), dels=0, ins=0)
    for name, (case, aln) in corpus.cases().items():
        nm, md_off, md, st = corpus.expected(name)
        mds = corpus.md_strings(name)
        lines = corpus.slot_lines(case, aln)
        assert len(mds) == 2 * len(case["hits"]) == len(nm), name
        for s, text in enumerate(mds):
            if s not in lines:
                assert text == b"" and nm[s] == 0, (name, s)
                continue
            r, rd, fwd, tid, x, words = lines[s]
            assert MD_RE.fullmatch(text), (name, s, text)
            seq = rd if fwd else VC.revcomp(rd)                                        # the line's SEQ as an oriented file holds it
            ref, judged, used = _rebuild(seq, words, text)
            t = case["seqs"][tid]
            span = sum(w >> 4 for w in words if w & 15 in (0, 2, 3, 7, 8))
            want = bytes((t[p:p + 1].upper()[0] if 0 <= p < len(t) and t[p:p + 1].upper().isalpha() and t[p] < 128 else 78) for p in range(x, x + span))
            assert ref == want, (name, s, text)
            assert judged == int(nm[s]), (name, s, text)
            if words:
                assert used == len(rd) or aln is None, (name, s)
            seen["slots"] += 1
            seen["runs"] |= {int(v) for v in re.findall(rb"[0-9]+", text)}
            seen["lens"].add(len(rd)); seen["nms"].add(int(nm[s]))
            seen["caret0"] += len(re.findall(rb"\^[A-Z]+0[A-Z]", text))
            seen["clip"] += int(any(w & 15 == 4 for w in words)); seen["over"] += int(x + span > len(t) and bool(words))
            seen["dels"] += sum(w & 15 == 2 for w in words); seen["ins"] += sum(w & 15 == 1 for w in words)
            seen["strands"].add(bool(fwd))
        seen["statuses"] |= set(case["hits"]["mate_status"].tolist())
        seen["max_md"] = max(seen["max_md"], st["max_md_bytes"]); seen["plain"] += st["slots_plain"]
        sizes = np.diff(md_off.astype(np.int64))
        assert st == dict(slots=len(lines), sum_nm=int(nm.sum()), md_bytes=len(md), max_md_bytes=int(sizes.max()) if len(sizes) else 0,
                          slots_plain=sum(1 for s, l in lines.items() if len(l[5]) == 1 and l[5][0] & 15 == 0 and nm[s] == 0)), name
    assert set(corpus.RUNS) <= seen["runs"] and set(corpus.LENGTHS) | {3000} <= seen["lens"] and set(corpus.MISMATCHES) | {3000} <= seen["nms"], seen
    assert seen["caret0"] >= 2 and seen["clip"] >= 20 and seen["over"] >= 6 and seen["max_md"] > 4096 and seen["plain"] >= 100, seen
    assert seen["statuses"] == {0, 1, 2, 3} and seen["strands"] == {True, False} and seen["dels"] >= 30 and seen["ins"] >= 30 and seen["slots"] > 3000, seen
    off = corpus.cases()["many_records"][0]["off"]
    assert set(corpus.NH_EDGES) | {0} <= set(np.diff(off.astype(np.int64)).tolist())


def test_nm_is_the_align_pass_nm(built):
    """for the slots the gapped alignment produced, nm is align_hits_host's"""
    n = 0
    for name in corpus.cases():
        if name.startswith("ag_") and name.endswith("_aligned"):
            want = AG.expected(name[3:-8], 3)
            nm = corpus.expected(name)[0]
            assert np.array_equal(nm, want[1]), name
            n += int((np.diff(want[2].astype(np.int64)) > 1).sum())
    assert n > 100


def _run_harness(L, case, aln, lanes, cap=None):
    ts, toff = VC.packed(case["seqs"])
    tl = np.array([len(x) for x in case["seqs"]], np.uint32)
    s1, o1 = VC.packed(case["r1"])
    s2, o2 = VC.packed(case["r2"]) if case["r2"] is not None else (None, None)
    n = len(case["hits"])
    cap = 1 << 20 if cap is None else cap
    nm, md_off, md, st = np.zeros(2 * n, np.uint32), np.zeros(2 * n + 1, np.uint64), np.zeros(max(cap, 1), np.uint8), np.zeros(5, np.uint64)
    p = lambda a: None if a is None else a.ctypes.data
    a_pos, a_off, a_ops = (None, None, None) if aln is None else (np.ascontiguousarray(aln[0], np.int32), np.ascontiguousarray(aln[2], np.uint64),
                                                                  np.ascontiguousarray(aln[3] if len(aln[3]) else [0], np.uint32))
    rc = L.mdh_tags(p(ts), p(toff), p(tl), len(tl), p(s1), p(o1), p(s2), p(o2), len(case["r1"]), p(case["hits"]), p(case["off"]), p(a_pos), p(a_off), p(a_ops),
                    lanes, p(nm), p(md_off), p(md), cap, p(st))
    return rc, nm, md_off, md, st


def test_mdfmt_equals_the_statement(built, harness):
    """over the whole corpus the harness, column by column and as a group of 16 lanes (and of 4, where a step is 64 columns), gives
    the statement's arrays and stats exactly"""
    from sailfish_amd import hits as H
    total = 0
    for name, (case, aln) in corpus.cases().items():
        nm, md_off, md, st = corpus.expected(name)
        for lanes in (0, 16, 4):
            rc, gn, go, gm, gst = _run_harness(harness, case, aln, lanes)
            what = (name, lanes)
            assert rc == len(md), what
            assert np.array_equal(go, md_off) and np.array_equal(gn, nm) and gm[:rc].tobytes() == md.tobytes(), what
            assert gst.tolist() == [st[key] for key in H.MDTAG_STATS], what
        total += len(md)
    assert total > 50000
    case = dict(corpus.cases()["edges_se"][0])
    bad = case["hits"].copy(); bad["tid"][[7, 3, 11]] = len(case["seqs"])
    case["hits"] = bad
    assert _run_harness(harness, case, None, 16)[0] == -(1 + 3)


def test_harness_runs_clean_under_sanitizers(built, tmp_path):
    """the same functions as a stand-alone program built with -fsanitize=address,undefined: every case of the corpus, every text and
    every MD in a block of exactly its size"""
    exe = str(tmp_path / "mdtag_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMDTAG_HARNESS_MAIN"] + WARN + [SRC, "-o", exe])
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for name in corpus.cases():
            f.write(corpus.blob(name))
    r = subprocess.run([exe, str(path)], text=True, capture_output=True)
    assert r.returncode == 0 and f"mdtag harness ok: {len(corpus.cases())} cases" in r.stdout, r.stdout + r.stderr


# ---- the serial writers take the tags ---------------------------------------------------------------------------------------------

def _write_harness(L, bam, case, aln, tags, read_names=None):
    from sailfish_amd import quantfile
    L.mdh_write.restype = C.c_int
    L.mdh_write.argtypes = [C.c_int, _P, _P, C.c_uint32, C.c_int] + [_P] * 2 + [C.c_uint32] + [_P] * 14
    names, _, _ = AG.sam_inputs(case)
    blob = lambda nn: tuple(np.frombuffer(bytes(b), np.uint8).copy() if not isinstance(b, np.ndarray) else b for b in quantfile.names_blob(nn))
    ref, ref_off = blob(names)
    qn, qn_off = blob(read_names) if read_names is not None else (None, None)
    paired = AG.is_paired(case)
    s1, o1 = VC.packed(case["r1"])
    s2, o2 = VC.packed(case["r2"]) if case["r2"] is not None else (None, None)
    p = lambda a: None if a is None else a.ctypes.data
    u64 = lambda a: None if a is None else np.ascontiguousarray(a).view(np.uint64)
    some = lambda a, dt: np.ascontiguousarray(a if len(a) else [0], dt)
    a_pos, a_off, a_ops = (None, None, None) if aln is None else (np.ascontiguousarray(aln[0], np.int32), u64(aln[2]), some(aln[3], np.uint32))
    t_nm, t_off, t_md = (None, None, None) if tags is None else (some(tags[0], np.uint32), u64(tags[1]), some(tags[2], np.uint8))
    o1, o2 = o1.view(np.int64), None if o2 is None else o2.view(np.int64)
    out = np.zeros(8, np.uint64)
    args = (bam, p(case["hits"]), p(case["off"]), len(case["r1"]), int(paired), p(ref), p(u64(ref_off)), len(names), p(qn), p(u64(qn_off)), p(s1), p(o1), p(s2), p(o2),
            p(a_pos), p(a_off), p(a_ops), p(t_nm), p(t_off), p(t_md))
    kind = L.mdh_write(*args, p(out), None)
    if kind:
        return kind, out, b""
    data = np.zeros(max(int(out[0]), 1), np.uint8)
    assert L.mdh_write(*args, p(out), p(data)) == 0 and not out[7]
    return 0, out, data[:int(out[0])].tobytes()


def _host_text(case, aln, tags, read_names=None):
    from sailfish_amd import samfile
    names, ref_len, seqs = AG.sam_inputs(case)
    return samfile._sam_text(names, ref_len, case["hits"], case["off"], read_names, seqs, oriented=True, alignments=aln, tags=tags), len(samfile.sam_header(names, ref_len))


def test_serial_writers_take_the_tags(built, harness):
    """csrc/samwfmt.h / csrc/bamwfmt.h with tags handed in against samfile._sam_text(tags=) and sam_to_bam of it, byte for byte behind
    the header; bam_to_sam(sam_to_bam(text)) is the text; read_sam_host / read_bam_host return the same records from the tagged and
    the untagged file; without tags the bytes are the statement's without them; every tagged line ends NM, MD, NH and the lines of a
    read without records carry none"""
    from sailfish_amd import samfile
    n_lines, types, round_trips = 0, set(), 0
    for name in corpus.WRITABLE:
        case, aln, tags = corpus.writable(name)
        text, head = _host_text(case, aln, tags)
        plain, _ = _host_text(case, aln, None)
        kind, out, got = _write_harness(harness, 0, case, aln, tags)
        assert kind == 0 and got == text[head:], name
        bam = samfile.sam_to_bam(text)
        kind, out, got = _write_harness(harness, 1, case, aln, tags)
        assert kind == 0 and got == bam[samfile._bam_header(bam)[2]:], name
        n_lines += int(out[1])
        reads = list(case["r1"]) + list(case["r2"] or [])
        if set(b"".join(reads)) <= set(b"ACGTN") and all(reads):      # (SEQ bytes that BAM's 4 bits keep; an empty SEQ reads back as '*')
            assert samfile.bam_to_sam(bam) == text, name
            round_trips += 1
        for bam_side in (0, 1):
            kind, _, got = _write_harness(harness, bam_side, case, aln, None)
            want = samfile.sam_to_bam(plain) if bam_side else plain
            assert kind == 0 and got == (want[samfile._bam_header(want)[2]:] if bam_side else want[head:]), (name, bam_side)
        nh = np.repeat(np.diff(case["off"].astype(np.int64)), np.diff(case["off"].astype(np.int64)))
        lines, plain_lines = text[head:].split(b"\n")[:-1], plain[head:].split(b"\n")[:-1]
        assert len(lines) == len(plain_lines)
        mapped = 0
        for l, pl in zip(lines, plain_lines):
            f = l.split(b"\t")
            assert f[:11] == pl.split(b"\t") and len(f) in (11, 14), name
            if int(f[1]) & 4:
                assert len(f) == 11, name
                continue
            assert [x[:5] for x in f[11:]] == [b"NM:i:", b"MD:Z:", b"NH:i:"] and MD_RE.fullmatch(f[12][5:]), (name, l)
            mapped += 1
            types |= {int(f[11][5:]), int(f[13][5:])}
        assert mapped == int(corpus.expected(name)[3]["slots"]) or aln is not None, name
        paired = AG.is_paired(case)
        tnames = [n.decode() for n in AG.sam_inputs(case)[0]]
        a, b = samfile.read_sam_host(text, tnames, paired), samfile.read_sam_host(plain, tnames, paired)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name
        a, b = samfile.read_bam_host(bam, tnames, paired), samfile.read_bam_host(samfile.sam_to_bam(plain), tnames, paired)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name
    assert n_lines > 3000 and {127, 128, 255, 256, 3000} <= types and round_trips >= 15
    # an unalignable slot still fails the batch as kind 1 at the lowest (read, record), in either format, tags or not
    case, aln = corpus.cases()["hand_ops"]
    tags = corpus.expected("hand_ops")[:3]
    for bam_side in (0, 1):
        kind, out, _ = _write_harness(harness, bam_side, case, aln, tags)
        assert kind == 1 and (int(out[5]), int(out[6])) == (8, 0)
    with pytest.raises(ValueError, match="read 8, record 0: "):
        _host_text(case, aln, tags)
    case, aln, tags = corpus.writable("edges_se")
    names, ref_len, seqs = AG.sam_inputs(case)
    for kw in (dict(oriented=False), dict(oriented=True, seqs=None)):
        with pytest.raises(ValueError, match="tags"):
            samfile._sam_text(names, ref_len, case["hits"], case["off"], None, kw.pop("seqs", seqs), tags=tags, **kw)
    with pytest.raises(ValueError, match="slots"):
        samfile._sam_text(names, ref_len, case["hits"], case["off"], None, seqs, oriented=True, tags=corpus.writable("runs_se")[2])


def test_a_tile_edge_falls_on_every_byte_of_the_tag_fields(built, harness):
    """the batch whose first QNAME is 1 .. 64 bytes long: the serial writers equal the statement for every length, and over the 64
    texts the 4 096-byte tile edges meet every byte offset of a line's tag fields"""
    from sailfish_amd import hits as H
    from sailfish_amd import samfile
    met, longest = set(), 0
    for n in range(1, 65):
        case, names = corpus.qnames_case(n)
        tags = H.md_tags_host(case["seqs"], case["hits"], case["off"], case["r1"], None)[:3]
        text, head = _host_text(case, None, tags, names)
        body = text[head:]
        kind, _, got = _write_harness(harness, 0, case, None, tags, names)
        assert kind == 0 and got == body, n
        if n in (1, 33, 64):
            bam = samfile.sam_to_bam(text)
            kind, _, got = _write_harness(harness, 1, case, None, tags, names)
            assert kind == 0 and got == bam[samfile._bam_header(bam)[2]:], n
        assert len(body) > 2 * 4096
        for edge in range(4096, len(body), 4096):
            start = body.rfind(b"\n", 0, edge) + 1
            line = body[start:body.index(b"\n", edge) + 1] if b"\n" in body[edge:] else body[start:]
            at = line.index(b"\tNM:i:")
            longest = max(longest, len(line) - at)
            if edge - start >= at:
                met.add(edge - start - at)
    assert longest >= 24 and set(range(longest)) <= met, (longest, sorted(met))


def test_mappings_tags_needs_an_oriented_mappings_file(built):
    """mappings_tags=True without write_mappings or without mappings_oriented: ValueError before anything is indexed (there is no
    device here)"""
    import sailfish_amd as sf
    for kw in (dict(), dict(write_mappings="m.sam"), dict(mappings_oriented=True), dict(write_mappings="m.sam", mappings_oriented=False)):
        with pytest.raises(ValueError, match="mappings_tags"):
            sf.mapper.quantify_reads(["t"], [b"ACGT" * 20], [b"ACGT" * 10], None, "U", "unused", mappings_tags=True, device="cuda", **kw)
        with pytest.raises(ValueError, match="mappings_tags"):
            sf.mapper.quantify_files("no.fa", "no.fq", None, "U", "unused", mappings_tags=True, device="cuda", **kw)
