"""Gapped alignment without a GPU: csrc/aligngfmt.h alone (tests/aligng_harness.cpp, g++ -Wall -Wextra -Werror; once more as a
stand-alone program under -fsanitize=address,undefined) against the Python statement hits.align_hits_host over the shared corpus
(tests/aligng_corpus.py), the issue's first thing to look at worked by hand, and what the statement promises: every CIGAR replays
over the mate and the transcript to its nm, S + M + I is the mate's length, and nm + clipped + trimmed D is gapped_edits_host's
edits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aligng_corpus as corpus
import verify_corpus as old_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "aligng_harness.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
_P = C.c_void_p


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("agh")), "libaligng_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.agh_align.restype = C.c_int64
    L.agh_align.argtypes = [_P, _P, _P, C.c_uint64, _P, _P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_int, _P, _P, _P, _P, C.c_uint64, _P, _P]
    return L


def _cigar(ops):
    return "".join("%d%s" % (int(w) >> 4, "MID?S"[int(w) & 15]) for w in ops)


def test_first_thing_to_look_at(built):
    """t[100:150] + t[152:202] recorded at pos 100 and at pos 102 (the seed behind the gap), max_indel = 3: both give pos 100 (POS
    101), 50M2D50M and nm == 2; with k = 1 the band cannot reach and the job is aligned on one side of the gap only"""
    from sailfish_amd import hits as H
    c = corpus.cases()["first_look"]
    pos, nm, op_off, ops, st, detail = corpus.expected("first_look", 3)
    assert pos.tolist() == [100, 0, 100, 0] and nm.tolist() == [2, 0, 2, 0] and op_off.tolist() == [0, 3, 3, 6, 6]
    assert _cigar(ops[:3]) == _cigar(ops[3:]) == "50M2D50M"
    assert st == dict(jobs=2, jobs_traced=2, unalignable=0, sum_nm=4, words=6, scratch_bytes=2 * 8 * 16 * 7) and detail[:, 2].tolist() == [2, 0, 2, 0]
    e, u = H.gapped_edits_host(c["seqs"], c["hits"], c["off"], c["r1"], c["r2"], 3)
    assert e[:, 0].tolist() == [2, 2] and min(u[:, 0]) > 25
    for k in (0, 16, -1):
        with pytest.raises(ValueError):
            H.align_hits_host(c["seqs"], c["hits"], c["off"], c["r1"], c["r2"], k)
    bad = c["hits"].copy(); bad["tid"][1] = 1
    with pytest.raises(ValueError, match="record 1 "):
        H.align_hits_host(c["seqs"], bad, c["off"], c["r1"], c["r2"], 3)
    # a mate that matches everywhere gets <len>M at pos from the rule itself, and an insertion is an I run
    t = c["seqs"][0]
    rec = np.array([(0, 40, 0, 0, 60, 0, 1, 0, 0, 0), (0, 40, 0, 0, 60, 0, 0, 0, 0, 0), (0, 100, 0, 0, 102, 0, 1, 0, 0, 0)], dtype=H.HIT_DTYPE)
    ins = t[100:150] + bytes([{65: 67, 67: 71, 71: 84, 84: 65}[t[150]]] * 2) + t[150:200]
    pos, nm, op_off, ops, st, detail = H.align_hits_host([t], rec, [0, 1, 2, 3], [t[40:100], old_corpus.revcomp(t[40:100]), ins], None, 2)
    assert [_cigar(ops[int(op_off[2 * i]):int(op_off[2 * i + 1])]) for i in range(3)] == ["60M", "60M", "50M2I50M"]
    assert pos[::2].tolist() == [40, 40, 100] and nm[::2].tolist() == [0, 0, 2] and st["jobs_traced"] == 1 and st["scratch_bytes"] == 8 * 16 * 7
    # hanging over the right end: the overhang is soft clip; wholly off the transcript: unalignable
    rec = np.array([(0, 370, 0, 0, 50, 0, 1, 0, 0, 0), (0, 1000, 0, 0, 50, 0, 1, 0, 0, 0), (0, -10, 0, 0, 50, 0, 1, 0, 0, 0)], dtype=H.HIT_DTYPE)
    over = t[370:400] + b"ACGTACGTACGTACGTACGT"
    pos, nm, op_off, ops, st, detail = H.align_hits_host([t], rec, [0, 1, 2, 3], [over, over, b"TTTTTTTTTT" + t[:40]], None, 3)
    assert [_cigar(ops[int(op_off[2 * i]):int(op_off[2 * i + 1])]) for i in range(3)] == ["30M20S", "", "10S40M"]
    assert pos[::2].tolist() == [370, 0, 0] and nm[::2].tolist() == [0, 0, 0] and st["unalignable"] == 1 and detail[::2].tolist() == [[20, 0, 20], [50, 0, 50], [10, 0, 10]]


def test_statement_properties(built):
    """over the corpus and every k of the grid: every CIGAR replays to its nm, S + M + I is the mate's length, nm + clipped + trimmed D
    is gapped_edits_host's edits (no D is ever trimmed), a slot without a job is empty, and the corpus holds what it must"""
    from sailfish_amd import hits as H
    seen = dict(jobs=0, unalignable=0, clipped=0, ins=0, dele=0, both_strands=set(), statuses=set(), lens=set(), n_base=0)
    for name, c in corpus.cases().items():
        lens = corpus.lengths(c)
        for k in corpus.KS:
            pos, nm, op_off, ops, st, detail = corpus.expected(name, k)
            e, u = H.gapped_edits_host(c["seqs"], c["hits"], c["off"], c["r1"], c["r2"], k)
            re = corpus.replay(c, (pos, nm, op_off, ops))
            n_ops = np.diff(op_off.astype(np.int64))
            job = lens >= 0
            assert not n_ops[~job].any() and not pos[~job].any() and not nm[~job].any(), (name, k)
            assert np.array_equal(detail[job, 2], e.reshape(-1)[job]), (name, k)
            assert np.array_equal(nm[job].astype(np.int64) + detail[job, 0] + detail[job, 1], detail[job, 2]), (name, k)
            assert not detail[:, 1].any(), (name, k)
            has = n_ops > 0
            assert np.array_equal(re[has, 0], nm[has].astype(np.int64)) and np.array_equal(re[has, 1], lens[has]), (name, k)
            assert np.array_equal(detail[job & ~has, 0], lens[job & ~has]) and not nm[~has].any() and not pos[~has].any(), (name, k)
            assert st["jobs"] == int(job.sum()) and st["unalignable"] == int((job & ~has).sum()) and st["sum_nm"] == int(nm.sum()) and st["words"] == len(ops)
            assert st["jobs_traced"] == int((u.reshape(-1)[job] > 0).sum())
            if k == 3:
                seen["jobs"] += st["jobs"]; seen["unalignable"] += int((job & ~has & (lens > 0)).sum()); seen["clipped"] += int((detail[has, 0] > 0).sum())
                seen["ins"] += int(((ops & 15) == H.CIGAR_I).sum()); seen["dele"] += int(((ops & 15) == H.CIGAR_D).sum())
                seen["lens"] |= set(lens[job].tolist())
                seen["statuses"] |= set(c["hits"]["mate_status"].tolist()); seen["both_strands"] |= set(c["hits"]["fwd"].tolist())
                seen["n_base"] += sum(b"N" in r for r in c["r1"])
    assert seen["jobs"] >= 600 and seen["unalignable"] >= 5 and seen["clipped"] >= 20 and seen["ins"] >= 30 and seen["dele"] >= 30, seen
    assert {0, 1, 15, 16, 17, 31, 32, 33, 2000} <= seen["lens"] and seen["statuses"] == {0, 1, 2, 3} and seen["both_strands"] == {0, 1} and seen["n_base"] >= 3, seen
    c = corpus.cases()["edges_pe"]
    assert (c["hits"]["pos"] < 0).any() and any(int(h["pos"]) + 5 > len(c["seqs"][int(h["tid"])]) for h in c["hits"])


def _run_harness(L, case, k, lanes, cap=None):
    ts, toff = old_corpus.packed(case["seqs"])
    tl = np.array([len(x) for x in case["seqs"]], np.uint32)
    s1, o1 = old_corpus.packed(case["r1"])
    s2, o2 = old_corpus.packed(case["r2"]) if case["r2"] is not None else (None, None)
    n = len(case["hits"])
    cap = 64 * n + 4096 if cap is None else cap
    pos, nm, op_off, ops = np.zeros(2 * n, np.int32), np.zeros(2 * n, np.uint32), np.zeros(2 * n + 1, np.uint64), np.zeros(max(cap, 1), np.uint32)
    extra, st = np.zeros(6 * n, np.uint64), np.zeros(6, np.uint64)
    p = lambda a: None if a is None else a.ctypes.data
    rc = L.agh_align(p(ts), p(toff), p(tl), len(tl), p(s1), p(o1), p(s2), p(o2), len(case["r1"]), p(case["hits"]), p(case["off"]), k, lanes, p(pos), p(nm),
                     p(op_off), p(ops), cap, p(extra), p(st))
    return rc, pos, nm, op_off, ops, extra.reshape(-1, 3), st


def test_aligngfmt_equals_the_statement(built, harness):
    """over the whole corpus, k in 1 2 3 7 8 15: the harness, in plain loops and as groups of 16 and 32 lanes (forward pass into
    scratch words, the walk counting and then writing from the right end), gives the statement's arrays and stats exactly"""
    from sailfish_amd import hits as H
    total = 0
    for name, case in corpus.cases().items():
        for k in corpus.KS:
            pos, nm, op_off, ops, st, detail = corpus.expected(name, k)
            for lanes in (0, 1):
                rc, gp, gn, go, gops, gx, gst = _run_harness(harness, case, k, lanes)
                what = (name, k, lanes)
                assert rc == len(ops), what
                assert np.array_equal(go, op_off) and np.array_equal(gp, pos) and np.array_equal(gn, nm) and np.array_equal(gops[:rc], ops), what
                assert np.array_equal(gx.astype(np.int64), detail), what
                assert gst.tolist() == [st[key] for key in H.ALIGNG_STATS], what
            total += len(ops)
    assert total > 5000
    case = dict(corpus.cases()["edges_se"])
    bad = case["hits"].copy(); bad["tid"][[7, 3, 11]] = len(case["seqs"])
    case["hits"] = bad
    assert _run_harness(harness, case, 3, 1)[0] == -(1 + 3)


def test_harness_runs_clean_under_sanitizers(built, tmp_path):
    """the same functions as a stand-alone program built with -fsanitize=address,undefined: every case of the corpus for every k, every
    text, scratch and operation list in a block of exactly its size"""
    exe = str(tmp_path / "aligng_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DALIGNG_HARNESS_MAIN"] + WARN + [SRC, "-o", exe])
    path = tmp_path / "cases.bin"
    n = 0
    with open(path, "wb") as f:
        for name in corpus.cases():
            for k in corpus.KS:
                f.write(corpus.blob(name, k)); n += 1
    r = subprocess.run([exe, str(path)], text=True, capture_output=True)
    assert r.returncode == 0 and f"aligng harness ok: {n} cases" in r.stdout, r.stdout + r.stderr


def _write_harness(L, bam, case, aln, oriented):
    from sailfish_amd import quantfile
    names, _, _ = corpus.sam_inputs(case)
    ref, ref_off = quantfile.names_blob(names)
    ref, ref_off = np.frombuffer(bytes(ref), np.uint8).copy() if not isinstance(ref, np.ndarray) else ref, np.ascontiguousarray(ref_off).view(np.uint64)
    paired = corpus.is_paired(case)
    s1, o1 = old_corpus.packed(case["r1"])
    s2, o2 = old_corpus.packed(case["r2"]) if case["r2"] is not None else (None, None)
    pos, _, op_off, ops = aln[:4]
    ops1 = ops if len(ops) else np.zeros(1, np.uint32)
    p = lambda a: None if a is None else a.ctypes.data
    o1, o2 = o1.view(np.int64), None if o2 is None else o2.view(np.int64)
    out = np.zeros(8, np.uint64)
    args = (bam, p(case["hits"]), p(case["off"]), len(case["r1"]), int(paired), p(ref), p(ref_off), len(names), p(s1), p(o1), p(s2), p(o2), int(oriented),
            p(pos), p(op_off), p(ops1))
    kind = L.agh_write(*args, p(out), None)
    if kind:
        return kind, out, b""
    data = np.zeros(max(int(out[0]), 1), np.uint8)
    assert L.agh_write(*args, p(out), p(data)) == 0 and not out[7]
    return 0, out, data[:int(out[0])].tobytes()


def test_serial_writers_take_an_alignment(built, harness):
    """csrc/samwfmt.h / csrc/bamwfmt.h with an alignment handed in against samfile._sam_text(alignments=) and sam_to_bam of it, byte
    for byte behind the header, plain and oriented; read_sam_host accepts the text; a slot without an operation fails the batch as
    kind 1 at the lowest (read, record); without an alignment the bytes are today's"""
    from sailfish_amd import samfile
    L = harness
    L.agh_write.restype = C.c_int
    L.agh_write.argtypes = [C.c_int, _P, _P, C.c_uint32, C.c_int, _P, _P, C.c_uint32, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P]
    n_lines = 0
    for name in corpus.cases():
        for k in (3, 8):
            case, aln = corpus.writable(name, k)
            names, ref_len, seqs = corpus.sam_inputs(case)
            for oriented in (False, True):
                text = samfile._sam_text(names, ref_len, case["hits"], case["off"], None, seqs, oriented=oriented, alignments=aln)
                head = len(samfile.sam_header(names, ref_len))
                kind, out, got = _write_harness(L, 0, case, aln, oriented)
                assert kind == 0 and got == text[head:], (name, k, oriented)
                bam = samfile.sam_to_bam(text)
                kind, out, got = _write_harness(L, 1, case, aln, oriented)
                assert kind == 0 and got == bam[samfile._bam_header(bam)[2]:], (name, k, oriented)
                n_lines += int(out[1])
            h, o = samfile.read_sam_host(text, [n.decode() for n in names], corpus.is_paired(case))[:2]
            assert len(o) == len(case["off"]), (name, k)                  # (accepted: every line parses, the reads are the reads)
            if not corpus.is_paired(case):                                # (a line a record; the pairing rules regroup a paired read's lines)
                assert np.array_equal(np.asarray(o).astype(np.int64), case["off"].astype(np.int64)), (name, k)
    assert n_lines > 4000
    # the first thing to look at: both records give the same line but for the secondary flag; without the alignment it is 100M
    case, aln = corpus.writable("first_look", 3)
    names, ref_len, seqs = corpus.sam_inputs(case)
    lines = samfile._sam_text(names, ref_len, case["hits"], case["off"], None, seqs, alignments=aln).split(b"\n")[2:4]
    assert [l.split(b"\t")[1:9] for l in lines] == [[b"0", b"t0", b"101", b"255", b"50M2D50M", b"*", b"0", b"0"]] * 2
    plain = samfile._sam_text(names, ref_len, case["hits"], case["off"], None, seqs).split(b"\n")[2:4]
    assert [l.split(b"\t")[3:6] for l in plain] == [[b"101", b"255", b"100M"], [b"103", b"255", b"100M"]]
    # unalignable slots: kind 1 at the lowest (read, record), in either format, and the statement raises for the same record
    for name in ("edges_pe", "edges_se"):
        case = corpus.cases()[name]
        aln = corpus.expected(name, 3)
        n_ops = np.diff(aln[2].astype(np.int64))
        bad = [(r, i - int(case["off"][r])) for r in range(len(case["off"]) - 1) for i in range(case["off"][r], case["off"][r + 1])
               if any(n_ops[2 * i + j] == 0 for j in range(2 if case["hits"][i]["mate_status"] == 3 else 1))]
        assert bad
        for bam in (0, 1):
            kind, out, _ = _write_harness(L, bam, case, aln, False)
            assert kind == 1 and (int(out[5]), int(out[6])) == bad[0], (name, bam)
        names, ref_len, seqs = corpus.sam_inputs(case)
        with pytest.raises(ValueError, match="read %d, record %d: " % bad[0]):
            samfile._sam_text(names, ref_len, case["hits"], case["off"], None, seqs, alignments=aln)
    with pytest.raises(ValueError, match="slots"):
        samfile._sam_text(names, ref_len, case["hits"], case["off"], None, seqs, alignments=corpus.expected("first_look", 3))


def test_python_surface_checks_max_indel(built):
    """align_hits raises for max_indel = 0, 16, -1 and 2.5 before any device work (there is no device here)"""
    from sailfish_amd import hits as H
    assert H.ALIGNG_STATS == ("jobs", "jobs_traced", "unalignable", "sum_nm", "words", "scratch_bytes")
    assert (H.CIGAR_M, H.CIGAR_I, H.CIGAR_D, H.CIGAR_S) == (0, 1, 2, 4)
    for bad in (0, 16, -1, 2.5):
        with pytest.raises(ValueError):
            H.align_hits(None, None, None, None, max_indel=bad)
    # mappings_gapped needs a mappings file, the validation pass and a band: ValueError before anything is indexed
    import sailfish_amd as sf
    for kw in (dict(validate_mappings=True, max_indel=3), dict(write_mappings="m.sam", max_indel=3), dict(write_mappings="m.sam", validate_mappings=True),
               dict(write_mappings="m.sam", validate_mappings=True, max_indel=0), dict(write_mappings="m.sam", validate_mappings=False, max_indel=3)):
        with pytest.raises(ValueError, match="mappings_gapped"):
            sf.mapper.quantify_reads(["t"], [b"ACGT" * 20], [b"ACGT" * 10], None, "U", "unused", mappings_gapped=True, device="cuda", **kw)
        with pytest.raises(ValueError, match="mappings_gapped"):
            sf.mapper.quantify_files("no.fa", "no.fq", None, "U", "unused", mappings_gapped=True, device="cuda", **kw)
    with pytest.raises(ValueError, match="align"):
        sf.mapper.QuasiIndex.map_reads(None, [b"ACGT"], validate=dict(align=True))
