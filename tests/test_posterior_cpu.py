"""The posterior pass and the ZW tag without a GPU: csrc/postfmt.h alone (tests/posterior_harness.cpp, g++ -Wall -Wextra -Werror; once
more as a stand-alone program under -fsanitize=address,undefined) against the Python statement hits.posteriors_host over the shared
corpus (tests/posterior_corpus.py), in the bits of p, the tokens and the bits of f32; the rule's small cases worked by hand; the
proof that the corpus tells a sum in another order apart; the host writers' statement samfile._sam_text(posteriors=) and sam_to_bam
of it, with the serial writers of csrc/samwfmt.h / csrc/bamwfmt.h held against them; and the options' ValueErrors."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import posterior_corpus as corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "posterior_harness.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
_P = C.c_void_p


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("posth")), "libposterior_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.ph_posteriors.restype = C.c_int64
    L.ph_posteriors.argtypes = [_P, _P, C.c_uint32, _P, C.c_uint64, C.c_int, _P, _P, _P, _P]
    L.ph_token.restype = C.c_int
    L.ph_token.argtypes = [C.c_uint32, _P]
    L.ph_write.restype = C.c_int
    L.ph_write.argtypes = [C.c_int, _P, _P, C.c_uint32, C.c_int, _P, _P, C.c_uint32] + [_P] * 8 + [C.c_int] + [_P] * 10
    return L


def _bits(a, dt):
    return np.ascontiguousarray(a).view(dt)


def test_the_rule_worked_by_hand(built):
    """the special reads of the corpus give the tokens the issue names; the counters of a batch small enough to count; every error of
    the statement names the lowest offender, the weights first; six digits survive a float32"""
    from sailfish_amd import hits as H
    assert H.POSTERIOR_STATS == corpus.STATS
    h, o, cls, special = corpus.batch()
    p, rec, f32, st = corpus.expected()
    toks = corpus.tokens(p)
    want = {name: t for name, _, t in corpus.SPECIAL}
    assert len(special) == len(corpus.SPECIAL)
    for r, name in special.items():
        assert toks[o[r]:o[r + 1]] == want[name], name
    assert [H.posterior_token(v) for v in rec] == toks
    assert np.array_equal(f32, np.array([float(t) for t in toks], np.float32))
    w = np.array([1.0, 3.0, 0.0, 2.0 ** -961])
    p, rec, f32, st = H.posteriors_host(corpus.records([0, 1, 2, 3, 2, 1, 1, 0]), [0, 2, 2, 4, 5, 8], w)
    assert p.tolist() == [0.25, 0.75, 0.5, 0.5, 1.0, 3 / 7, 3 / 7, 1 / 7] and corpus.tokens(p)[-3:] == ["0.428571", "0.428571", "0.142857"]
    assert st == dict(reads=5, reads_mapped=4, reads_multi=3, records=8, reads_flat=2, records_zero=0, max_records=3)
    p, _, _, st = H.posteriors_host(corpus.records([0, 1]), [0, 2], [1e-17, 1.0])
    assert p.tolist() == [0.0, 1.0] and st["records_zero"] == 1 and st["reads_flat"] == 0
    p, _, _, st = H.posteriors_host(corpus.records([0, 1]), [0, 2], [2.0 ** -56, 1.0])             # x / S rounds to 2^-56 itself: kept
    assert p[0] == 2.0 ** -56 and st["records_zero"] == 0
    assert H.posteriors_host(corpus.records([]), [0], [1.0])[3] == dict.fromkeys(H.POSTERIOR_STATS, 0)
    assert H.posteriors_host(corpus.records([]), [0, 0, 0], [])[3]["reads"] == 2
    for bad in (-1.0, float("nan"), float("inf"), 2.0 ** 961, -2.0 ** -1074):
        with pytest.raises(ValueError, match="transcript 2 "):
            H.posteriors_host(corpus.records([0, 9]), [0, 2], [1.0, 1.0, bad, 1.0, bad])
    assert H.posteriors_host(corpus.records([0]), [0, 1], [2.0 ** 960])[0].tolist() == [1.0]
    with pytest.raises(ValueError, match="record 1 "):
        H.posteriors_host(corpus.records([0, 3, 1, 4]), [0, 4], [1.0, 1.0, 1.0])
    rng = np.random.default_rng(5)
    for v in np.concatenate([rng.random(10000), 10.0 ** rng.uniform(-16.8, 0, 10000)]).tolist():
        t = "%g" % v
        assert "%g" % float(np.float32(float(t))) == t and H.posterior_token(H.posterior_record(v)) == t


def test_the_sum_has_the_shape_the_rule_says_and_the_corpus_tells_another_apart(built):
    """post_sum_host equals the tree truncated to P leaves for every n <= P, and the strided accumulators for n > 64, written out
    here once more; and a serial left-to-right sum changes p in at least one read of every size class above 2 -- else the bit
    equalities of the other tests would prove nothing"""
    from sailfish_amd import hits as H

    def tree(a):
        a = list(a)
        k = len(a) // 2
        while k:
            a = [a[j] + a[j + k] for j in range(k)]
            k //= 2
        return a[0]

    h, o, cls, _ = corpus.batch()
    p = corpus.expected()[0]
    w = corpus.weights()
    x_all = np.where(w < 2.0 ** -960, 0.0, w)[h["tid"]]
    differs = dict.fromkeys([n for n in corpus.SIZES if n > 2], 0)
    seen = 0
    for r, n in enumerate(cls.tolist()):
        if n < 1:
            continue
        x = x_all[o[r]:o[r + 1]].tolist()
        P = next(q for q in (1, 2, 4, 8, 16, 32, 64) if q >= min(n, 64))
        acc = [0.0] * P
        for i, v in enumerate(x):
            acc[i % 64 if n > 64 else i] += v
        s = H.post_sum_host(np.array(x))
        assert s == tree(acc), (r, n)
        serial = 0.0
        for v in x:
            serial += v
        if n > 2 and s > 0 and not np.array_equal(np.array(x) / serial, np.array(x) / s):
            differs[n] += 1
        seen += 1
        assert np.array_equal(np.where(np.array(x) / s < 2.0 ** -56, 0.0, np.array(x) / s), p[o[r]:o[r + 1]]) if s > 0 else True
    assert seen == corpus.READS_PER_SIZE * (len(corpus.SIZES) - 1) == 440
    assert all(differs.values()), differs


def _run(L, hits, off, w, layout):
    hits, off, w = np.ascontiguousarray(hits), np.ascontiguousarray(off, np.uint32), np.ascontiguousarray(w, np.float64)
    n = len(hits)
    p, rec, f32, st = np.full(n + 1, 7.0), np.full(n + 1, 7, np.uint32), np.full(n + 1, 7.0, np.float32), np.zeros(7, np.uint64)
    rc = L.ph_posteriors(hits.ctypes.data, off.ctypes.data, len(off) - 1, w.ctypes.data, len(w), layout, p.ctypes.data, rec.ctypes.data, f32.ctypes.data, st.ctypes.data)
    assert p[n] == 7.0 and rec[n] == 7 and f32[n] == 7.0
    return rc, p[:n], rec[:n], f32[:n], st


def test_postfmt_equals_the_statement(built, harness):
    """over the corpus the header, in the statement's form and in the layout the kernel gives the work, equals posteriors_host in the
    bits of p, in the tokens placed from rec, in the bits of f32 and in every counter; its errors name the statement's offenders and
    leave the outputs untouched"""
    from sailfish_amd import hits as H
    h, o, _, _ = corpus.batch()
    p, rec, f32, st = corpus.expected()
    buf = C.create_string_buffer(16)
    for layout in (0, 1):
        rc, gp, grec, gf32, gst = _run(harness, h, o, corpus.weights(), layout)
        assert rc == 0, layout
        assert np.array_equal(_bits(gp, np.uint64), _bits(p, np.uint64)), layout
        assert np.array_equal(grec, rec) and np.array_equal(_bits(gf32, np.uint32), _bits(f32, np.uint32)), layout
        assert gst.tolist() == [st[k] for k in H.POSTERIOR_STATS], layout
    toks = corpus.tokens(p)
    for v, t in zip(rec.tolist(), toks):
        n = harness.ph_token(v, buf)
        assert buf.raw[:n].decode() == t
    assert st["reads_flat"] >= 1 and st["records_zero"] >= 3 and st["max_records"] == 1000 and {len(t) for t in toks} >= {1, 8, 11}
    for layout in (0, 1):
        for bad in (-1.0, float("nan"), float("inf"), 2.0 ** 961):
            w = corpus.weights().copy()
            w[[31, 12, 44]] = bad
            rc, gp, grec, _, _ = _run(harness, h, o, w, layout)
            assert rc == 1 + 12 and (gp == 7.0).all() and (grec == 7).all(), (layout, bad)
        hb = h.copy()
        hb["tid"][[900, 77, 5000]] = corpus.N_REFS
        rc, gp, _, _, _ = _run(harness, hb, o, corpus.weights(), layout)
        assert rc == -(1 + 77) and (gp == 7.0).all(), layout
        w = corpus.weights().copy()
        w[9] = -1.0
        assert _run(harness, hb, o, w, layout)[0] == 1 + 9                     # the weights are checked first
        assert _run(harness, h[:0], o[:1], w[:0], layout)[0] == 0              # no reads, no transcripts


def test_harness_runs_clean_under_sanitizers(built, tmp_path):
    """the same functions as a stand-alone program built with -fsanitize=address,undefined and run directly: the corpus's batch, every
    array in a block of exactly its size"""
    exe = str(tmp_path / "posterior_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPOSTERIOR_HARNESS_MAIN"] + WARN + [SRC, "-o", exe])
    path = tmp_path / "batch.bin"
    path.write_bytes(corpus.blob())
    r = subprocess.run([exe, str(path)], text=True, capture_output=True)
    h, o, _, _ = corpus.batch()
    assert r.returncode == 0 and f"posterior harness ok: {len(o) - 1} reads, {len(h)} records" in r.stdout, r.stdout + r.stderr


# ---- the writers ---------------------------------------------------------------------------------------------------------------------

def _host_text(case, aln, tags, post, read_names=None, oriented=True, quals=None):
    import aligng_corpus as AG
    from sailfish_amd import samfile
    names, ref_len, seqs = AG.sam_inputs(case)
    return samfile._sam_text(names, ref_len, case["hits"], case["off"], read_names, seqs, oriented=oriented, alignments=aln, tags=tags, posteriors=post, quals=quals), \
        len(samfile.sam_header(names, ref_len))


def _case_quals(case):
    import aligng_corpus as AG
    q1 = corpus.quals(case["r1"])
    if not AG.is_paired(case):
        return q1, (q1, None)
    q2 = corpus.quals(case["r2"])
    return list(zip(q1, q2)), (q1, q2)


def _serial(L, bam, case, aln, tags, post, read_names=None, oriented=1, quals=(None, None)):
    import aligng_corpus as AG
    import verify_corpus as VC
    from sailfish_amd import quantfile
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
    flat = lambda q: None if q is None else np.frombuffer(b"".join(q) + b"!", np.uint8).copy()
    a_pos, a_off, a_ops = (None, None, None) if aln is None else (np.ascontiguousarray(aln[0], np.int32), u64(aln[2]), some(aln[3], np.uint32))
    t_nm, t_off, t_md = (None, None, None) if tags is None else (some(tags[0], np.uint32), u64(tags[1]), some(tags[2], np.uint8))
    z_rec, z_f32 = (None, None) if post is None else (some(post[1], np.uint32), some(post[2], np.float32))
    q1, q2 = flat(quals[0]), flat(quals[1])
    o1, o2 = o1.view(np.int64), None if o2 is None else o2.view(np.int64)
    out = np.zeros(5, np.uint64)
    args = (bam, p(case["hits"]), p(case["off"]), len(case["r1"]), int(paired), p(ref), p(u64(ref_off)), len(names), p(qn), p(u64(qn_off)), p(s1), p(o1), p(s2), p(o2),
            p(q1), p(q2), oriented, p(a_pos), p(a_off), p(a_ops), p(t_nm), p(t_off), p(t_md), p(z_rec), p(z_f32))
    assert L.ph_write(*args, p(out), None) == 0 and not out[3]
    data = np.zeros(max(int(out[0]), 1), np.uint8)
    assert L.ph_write(*args, p(out), p(data)) == 0 and not out[3]
    return data[:int(out[0])].tobytes()


def _bam_records(bam):
    from sailfish_amd import samfile
    at, out = samfile._bam_header(bam)[2], []
    while at < len(bam):
        n = struct.unpack_from("<i", bam, at)[0]
        out.append(bam[at + 4:at + 4 + n])
        at += 4 + n
    assert at == len(bam)
    return out


def test_the_host_statement_and_the_serial_writers(built, harness):
    """_sam_text(posteriors=): a mapped line ends ZW:f:<"%g" % p of its record>, behind NM, MD and NH where tags are given, both lines
    of a pair alike, and an unmapped line carries nothing; without the argument the text is the one it was; sam_to_bam ends the
    record Z W f and the float32's four bytes, counted by block_size.  The serial writers of csrc/samwfmt.h / csrc/bamwfmt.h, given
    rec and f32, write the same bytes -- with nothing else, with qualities and tags, with a gapped alignment and tags, oriented or not"""
    from sailfish_amd import samfile
    lines = 0
    for name in corpus.WRITER_CASES:
        case, aln, tags, post = corpus.writable(name)
        per_read, mates = _case_quals(case)
        p = post[0]
        for kw in (dict(aln=None, tags=None), dict(aln=aln, tags=tags, quals=per_read), dict(aln=aln, tags=None, oriented=False)):
            ser = dict(quals=mates) if "quals" in kw else {}
            text, head = _host_text(case, post=post[:1], **kw)
            plain, _ = _host_text(case, post=None, **kw)
            assert re.sub(rb"\tZW:f:[^\t\n]*", b"", text) == plain, name
            rec_of_line = [h for h in range(len(case["hits"])) for _ in range(2 if case["hits"]["mate_status"][h] == 3 else 1)]
            at = 0
            for l in text[head:].split(b"\n")[:-1]:
                f = l.split(b"\t")
                if int(f[1]) & 4:
                    assert len(f) == 11, name
                    continue
                want = [b"NM:i:", b"MD:Z:", b"NH:i:", b"ZW:f:"] if kw["tags"] is not None else [b"ZW:f:"]
                assert [x[:5] for x in f[11:]] == want and f[-1][5:] == b"%g" % p[rec_of_line[at]], (name, l)
                at += 1
            assert at == len(rec_of_line)
            lines += at
            bam = samfile.sam_to_bam(text)
            o = int(kw.get("oriented", True))
            assert _serial(harness, 0, case, kw["aln"], kw["tags"], post, oriented=o, **ser) == text[head:], (name, kw.keys())
            assert _serial(harness, 1, case, kw["aln"], kw["tags"], post, oriented=o, **ser) == bam[samfile._bam_header(bam)[2]:], (name, kw.keys())
            assert _serial(harness, 0, case, kw["aln"], kw["tags"], None, oriented=o, **ser) == plain[head:], name
            mapped = [r for r in _bam_records(bam) if not struct.unpack_from("<H", r, 14)[0] & 4]
            before = [r for r in _bam_records(samfile.sam_to_bam(plain)) if not struct.unpack_from("<H", r, 14)[0] & 4]
            assert len(mapped) == len(before) == len(rec_of_line)
            for r, b, h in zip(mapped, before, rec_of_line):
                assert len(r) == len(b) + 7 and r[:-7] == b and r[-7:] == b"ZWf" + struct.pack("<f", float("%g" % p[h])) == b"ZWf" + post[2][h].tobytes(), name
    assert lines > 300
    case, aln, tags, post = corpus.writable("runs_se")
    with pytest.raises(ValueError, match="posteriors of"):
        _host_text(case, None, None, (post[0][:-1],))


def test_a_tile_edge_falls_on_every_byte_of_the_zw_field(built, harness):
    """the batch whose first QNAME is 1 .. 64 bytes long, tagged, with tokens of 1, 8 and 11 bytes: the serial writers equal the statement
    (a few lengths; the device test takes every one), and over the 64 texts the 4 096-byte tile edges meet every byte offset of the ZW
    field"""
    from sailfish_amd import hits as H
    from sailfish_amd import samfile
    for token in corpus.TOKENS_AT_THE_EDGE:
        met, longest = set(), 0
        for n in range(1, 65):
            case, names, p = corpus.qnames_case(n, token)
            tags = H.md_tags_host(case["seqs"], case["hits"], case["off"], case["r1"], None)[:3]
            text, head = _host_text(case, None, tags, (p,), names)
            body = text[head:]
            if n in (1, 33, 64):
                post = (p, np.array([H.posterior_record(v) for v in p], np.uint32), np.array([float(token)] * len(p), np.float32))
                assert _serial(harness, 0, case, None, tags, post, names) == body, n
                bam = samfile.sam_to_bam(text)
                assert _serial(harness, 1, case, None, tags, post, names) == bam[samfile._bam_header(bam)[2]:], n
            assert len(body) > 2 * 4096
            for edge in range(4096, len(body), 4096):
                start = body.rfind(b"\n", 0, edge) + 1
                line = body[start:body.index(b"\n", edge) + 1] if b"\n" in body[edge:] else body[start:]
                at = line.index(b"\tZW:f:")
                longest = max(longest, len(line) - at)
                if edge - start >= at:
                    met.add(edge - start - at)
        assert longest == 7 + len(token) and set(range(longest)) <= met, (token, longest, sorted(met))


def test_mappings_posteriors_needs_a_mappings_file(built):
    """mappings_posteriors=True without write_mappings: ValueError before anything is indexed (there is no device here), whatever
    else is asked for"""
    import sailfish_amd as sf
    for kw in (dict(), dict(mappings_oriented=True), dict(mappings_format="bam"), dict(validate_mappings=True)):
        with pytest.raises(ValueError, match="mappings_posteriors"):
            sf.mapper.quantify_reads(["t"], [b"ACGT" * 20], [b"ACGT" * 10], None, "U", "unused", mappings_posteriors=True, device="cuda", **kw)
        with pytest.raises(ValueError, match="mappings_posteriors"):
            sf.mapper.quantify_files("no.fa", "no.fq", None, "U", "unused", mappings_posteriors=True, device="cuda", **kw)
