"""Gapped alignment on the device (csrc/align_gapped.hip: sfgpu_hits_align_gapped; hits.align_hits) against the Python statement
hits.align_hits_host: array for array over the shared corpus (tests/aligng_corpus.py) for both group widths, the contract's shapes
and errors, and a scratch cap small enough to force many slices; the device writers with an alignment handed in
(samfile.SamDeviceWriter.write(alignments=): "sam", "sam.gz", "bam" and the sorted "bam" with its index) against the host statements
samfile._sam_text(alignments=), sam_to_bam, write_bam(sort="coordinate") and build_bai; and mappings_gapped= of
mapper.quantify_reads end to end."""
import ctypes as C
import gzip
import io
import os

import numpy as np
import pytest

import aligng_corpus as corpus

pytestmark = pytest.mark.gpu


def _index(case, gpu):
    import sailfish_amd as sf
    return sf.mapper.QuasiIndex(case["seqs"], device=gpu)


def _device(case, gpu):
    import torch
    hits = torch.from_numpy(case["hits"].view(np.uint8).reshape(-1).copy()).to(gpu)
    off = torch.from_numpy(case["off"].view(np.int32).copy()).to(gpu)
    return hits, off


def _reads(case, gpu, lead1=b"", lead2=b""):
    """the case's reads packed on the device; a lead shifts every read to an offset that is no multiple of 16"""
    import sailfish_amd as sf
    out = []
    for reads, lead in ((case["r1"], lead1), (case["r2"], lead2)):
        if reads is None:
            out.append(None)
            continue
        b, o = sf.mapper.pack_sequences(([lead] if lead else []) + list(reads))
        out.append((b.to(gpu), (o[1:] if lead else o).contiguous().to(gpu)))
    return out


def _numpy(pos, nm, op_off, ops):
    return pos.cpu().numpy(), nm.cpu().numpy().view(np.uint32), op_off.cpu().numpy().view(np.uint64), ops.cpu().numpy().view(np.uint32)


def _same(got, want, what, scratch=True):
    pos, nm, op_off, ops, st = got
    assert np.array_equal(op_off, want[2]), what
    assert np.array_equal(pos, want[0]) and np.array_equal(nm, want[1]) and np.array_equal(ops, want[3]), what
    drop = () if scratch else ("scratch_bytes",)
    assert {k: v for k, v in st.items() if k not in drop} == {k: v for k, v in want[4].items() if k not in drop}, (what, st, want[4])


def _cigar(ops):
    return "".join("%d%s" % (int(w) >> 4, "MID?S"[int(w) & 15]) for w in ops)


def test_first_thing_to_look_at(gpu):
    """t[100:150] + t[152:202] recorded at pos 100 and at pos 102 (the seed behind the gap), max_indel = 3: both slots give pos 100,
    one D run of length 2 between M runs that sum to 100, nm == 2; the device writers then print the same line for both, POS 101 and
    50M2D50M, and without an alignment the two lines of today: 100M at 101 and at 103"""
    from sailfish_amd import hits as H
    from sailfish_amd import samfile
    c = corpus.cases()["first_look"]
    idx = _index(c, gpu)
    pos, nm, op_off, ops, st = H.align_hits(idx, c["hits"], c["off"], c["r1"], max_indel=3)
    pos, nm, op_off, ops = _numpy(pos, nm, op_off, ops)
    assert pos.tolist() == [100, 0, 100, 0] and nm.tolist() == [2, 0, 2, 0] and op_off.tolist() == [0, 3, 3, 6, 6]
    assert _cigar(ops[:3]) == _cigar(ops[3:]) == "50M2D50M"
    assert st == dict(jobs=2, jobs_traced=2, unalignable=0, sum_nm=4, words=6, scratch_bytes=2 * 8 * 16 * 7)
    idx.close()
    names, ref_len, seqs = corpus.sam_inputs(c)
    head = samfile.sam_header(names, ref_len)
    read = c["r1"][0]
    line = lambda q, p, cigar: b"\t".join([q, b"0", b"t0", b"%d" % p, b"255", cigar, b"*", b"0", b"0", read, b"*"]) + b"\n"
    for aln, body in (((pos, nm, op_off, ops), line(b"r0", 101, b"50M2D50M") + line(b"r1", 101, b"50M2D50M")),
                      (None, line(b"r0", 101, b"100M") + line(b"r1", 103, b"100M"))):
        assert samfile._sam_text(names, ref_len, c["hits"], c["off"], None, seqs, alignments=aln) == head + body
        assert _written(c, aln, gpu, "sam")[0] == head + body
        assert gzip.decompress(_written(c, aln, gpu, "sam.gz")[0]) == head + body
        assert gzip.decompress(_written(c, aln, gpu, "bam")[0]) == samfile.sam_to_bam(head + body)


@pytest.mark.parametrize("name", ["pe_indel", "se_indel", "edges_pe", "edges_se", "indels_pe", "indels_se", "first_look", "homopolymers", "long",
                                  "power_of_two"])
def test_device_equals_the_statement(gpu, name):
    """every case of the corpus, max_indel 1 2 3 7 (groups of 16 lanes) 8 15 (of 32): pos, nm, op_off, ops and the stats are the
    statement's; once more with every read at an offset that is no multiple of 16"""
    from sailfish_amd import hits as H
    case = corpus.cases()[name]
    idx = _index(case, gpu)
    d_hits, d_off = _device(case, gpu)
    r1, r2 = _reads(case, gpu)
    s1, s2 = _reads(case, gpu, b"xyz", b"NNNNNNN")
    assert any(int(x) % 16 for x in s1[1].cpu().numpy())
    for k in corpus.KS:
        want = corpus.expected(name, k)
        for a, b in ((r1, r2), (s1, s2)):
            pos, nm, op_off, ops, st = H.align_hits(idx, d_hits, d_off, a, b, max_indel=k)
            _same((*_numpy(pos, nm, op_off, ops), st), want, (name, k))
    idx.close()


def test_a_tiny_scratch_cap_changes_nothing(gpu):
    """the cap bounds memory, not results: 4 KiB forces a slice every few jobs (and the mate of 2 000 bases, 16 000 bytes at 16 lanes,
    runs alone above it); 1 byte gives every traced job a slice of its own"""
    from sailfish_amd import hits as H
    for name, caps in (("pe_indel", (4096, 40000)), ("long", (4096,)), ("homopolymers", (1, 2000))):
        case = corpus.cases()[name]
        idx = _index(case, gpu)
        d_hits, d_off = _device(case, gpu)
        r1, r2 = _reads(case, gpu)
        for k in (3, 8):
            want = corpus.expected(name, k)
            largest = max(8 * (16 if k <= 7 else 32) * ((n + 15) // 16) for n in corpus.lengths(case))
            for cap in caps:
                pos, nm, op_off, ops, st = H.align_hits(idx, d_hits, d_off, r1, r2, max_indel=k, scratch_cap_bytes=cap)
                _same((*_numpy(pos, nm, op_off, ops), st), want, (name, k, cap), scratch=False)
                assert 0 < st["scratch_bytes"] <= max(cap, largest) and st["scratch_bytes"] < want[4]["scratch_bytes"], (name, k, cap, st)
        idx.close()


def _raw(idx, s1, o1, s2, o2, n_reads, d_hits, d_off, k, pos, nm, op_off, ops, cap, n_ops=True, stats=True, opts=True, index=True, scratch=0):
    """sfgpu_hits_align_gapped itself -> (rc, n_ops, stats)"""
    import torch
    from sailfish_amd import _lib
    o = _lib.AlignGOpts(k, 0, scratch)
    st = _lib.AlignGStats()
    n = C.c_uint64(12345)
    with torch.cuda.device(idx.device):
        torch.cuda.synchronize()
        rc = _lib.lib().sfgpu_hits_align_gapped(idx._h if index else None, _lib.ptr(s1), _lib.ptr(o1), _lib.ptr(s2), _lib.ptr(o2), n_reads, _lib.ptr(d_hits),
                                                _lib.ptr(d_off), C.byref(o) if opts else None, _lib.ptr(pos), _lib.ptr(nm), _lib.ptr(op_off), _lib.ptr(ops), cap,
                                                C.byref(n) if n_ops else None, C.byref(st) if stats else None, _lib.current_stream_ptr())
        torch.cuda.synchronize()
    return rc, n.value, st.as_dict()


def test_shapes_and_errors_of_the_contract(gpu):
    """no records; n_reads == 0; room for too few operations: SFGPU_ERR_RANGE, the need reported exactly, the outputs untouched, and
    align_hits repeats the call once; tid >= M: SFGPU_ERR_RANGE naming the lowest record; null pointers, max_indel outside 1 .. 15 and
    mate 2 in a single-end batch: SFGPU_ERR_INVALID, the outputs untouched"""
    import torch
    from sailfish_amd import _lib
    from sailfish_amd import hits as H
    case = corpus.cases()["edges_pe"]
    want = corpus.expected("edges_pe", 3)
    idx = _index(case, gpu)
    d_hits, d_off = _device(case, gpu)
    (s1, o1), (s2, o2) = _reads(case, gpu)
    R, n = len(case["r1"]), len(case["hits"])
    zero = dict.fromkeys(H.ALIGNG_STATS, 0)
    need = len(want[3])
    assert need > 4 * n // 3                                          # (more than a word a job: clips and gaps)
    fresh = lambda: [torch.full((m,), 0x5A, dtype=torch.uint8, device=gpu) for m in (2 * n * 4, 2 * n * 4, (2 * n + 1) * 8, need * 4)]
    untouched = lambda ts: all(bool((t == 0x5A).all().item()) for t in ts)
    # no records at all, and no reads
    none_o = torch.zeros(R + 1, dtype=torch.int32, device=gpu)
    pos, nm, op_off, ops, st = H.align_hits(idx, torch.zeros(0, dtype=torch.uint8, device=gpu), none_o, (s1, o1), (s2, o2), max_indel=3)
    assert pos.numel() == 0 and nm.numel() == 0 and ops.numel() == 0 and op_off.tolist() == [0] and st == zero
    one = torch.full((1,), 7, dtype=torch.int64, device=gpu)
    rc, n_ops, st = _raw(idx, None, None, None, None, 0, None, None, 3, None, None, one, None, 0)
    assert rc == 0 and n_ops == 0 and one.item() == 0 and st == zero
    # the whole thing, raw, with exactly the room it needs
    outs = fresh()
    rc, n_ops, st = _raw(idx, s1, o1, s2, o2, R, d_hits, d_off, 3, *outs, need)
    assert rc == 0 and n_ops == need and st == want[4]
    got = [t.cpu().numpy().view(dt) for t, dt in zip(outs, (np.int32, np.uint32, np.uint64, np.uint32))]
    assert all(np.array_equal(g, w) for g, w in zip(got, want[:4]))
    # one word too few, and none
    for cap in (need - 1, 0):
        outs = fresh()
        rc, n_ops, st = _raw(idx, s1, o1, s2, o2, R, d_hits, d_off, 3, *outs[:3], outs[3] if cap else None, cap)
        assert rc == _lib.ERR_RANGE and n_ops == need and untouched(outs), cap
    # tid >= M
    bad = case["hits"].copy()
    bad["tid"][[40, 17, 99]] = len(case["seqs"])
    bad_hits = torch.from_numpy(bad.view(np.uint8).reshape(-1).copy()).to(gpu)
    outs = fresh()
    for k in (3, 15):
        rc, _, _ = _raw(idx, s1, o1, s2, o2, R, bad_hits, d_off, k, *outs, need)
        assert rc == _lib.ERR_RANGE and b"record 17 " in _lib.lib().sfgpu_last_error() and untouched(outs)
    with pytest.raises(_lib.SfgpuError, match="record 17 "):
        H.align_hits(idx, bad_hits, d_off, (s1, o1), (s2, o2), max_indel=3)
    args = dict(idx=idx, s1=s1, o1=o1, s2=s2, o2=o2, n_reads=R, d_hits=d_hits, d_off=d_off, k=3, pos=outs[0], nm=outs[1], op_off=outs[2], ops=outs[3], cap=need)
    for change in (dict(index=False), dict(opts=False), dict(n_ops=False), dict(stats=False), dict(op_off=None), dict(s1=None), dict(o1=None), dict(o2=None),
                   dict(d_off=None), dict(d_hits=None), dict(pos=None), dict(nm=None), dict(ops=None), dict(k=0), dict(k=16), dict(k=0xFFFFFFFF),
                   dict(s2=None, o2=None)):                           # (the last: records name mate 2)
        rc, _, _ = _raw(**{**args, **change})
        assert rc == _lib.ERR_INVALID, change
    assert b"mate 2" in _lib.lib().sfgpu_last_error() and untouched(outs)
    for k in (0, 16, -1):
        with pytest.raises(ValueError):
            H.align_hits(idx, d_hits, d_off, (s1, o1), (s2, o2), max_indel=k)
    idx.close()
    # align_hits sizes the operations at two words a slot and repeats the call once: a batch of clipped and gapped jobs that needs more
    t = corpus.cases()["first_look"]["seqs"][0]
    read = b"GGGGGGGG" + t[:30] + t[32:60] + t[62:90] + b"CC" + t[90:120]      # 8S 30M 2D 28M 2D 28M 2I 30M at pos 0
    rec = np.array([(0, -8, 0, 0, len(read), 0, 1, 0, 0, 0)], dtype=H.HIT_DTYPE)
    idx = _index(dict(seqs=[t]), gpu)
    pos, nm, op_off, ops, st = H.align_hits(idx, rec, np.array([0, 1], np.uint32), [read], max_indel=15)
    wp, wn, wo, wops, wst, _ = H.align_hits_host([t], rec, [0, 1], [read], None, 15)
    assert len(wops) > 4
    _same((*_numpy(pos, nm, op_off, ops), st), (wp, wn, wo, wops, wst), "retry")
    idx.close()


# ---- the writers take an alignment ------------------------------------------------------------------------------------------------

def _aln_device(aln, gpu):
    import torch
    pos, nm, op_off, ops = aln[:4]
    return (torch.from_numpy(pos.copy()).to(gpu), torch.from_numpy(nm.view(np.int32).copy()).to(gpu), torch.from_numpy(op_off.view(np.int64).copy()).to(gpu),
            torch.from_numpy(ops.view(np.int32).copy()).to(gpu))


def _written(case, aln, gpu, fmt, oriented=False, sort=None, chunk_bytes=0, cuts=None):
    """the case through SamDeviceWriter in one batch, or in the batches cut at the reads `cuts` -> (the file's bytes, the index's)"""
    from sailfish_amd import samfile
    names, ref_len, _ = corpus.sam_inputs(case)
    paired = corpus.is_paired(case)
    f, x = io.BytesIO(), io.BytesIO()
    w = samfile.SamDeviceWriter(f, names, ref_len, paired, format=fmt, oriented=oriented, sort=sort, chunk_bytes=chunk_bytes, index=x if sort else None)
    edges = [0] + list(cuts or []) + [len(case["r1"])]
    for a, b in zip(edges[:-1], edges[1:]):
        h0, h1 = int(case["off"][a]), int(case["off"][b])
        part = dict(seqs=case["seqs"], r1=case["r1"][a:b], r2=None if case["r2"] is None else case["r2"][a:b], hits=case["hits"][h0:h1],
                    off=(case["off"][a:b + 1] - case["off"][a]).astype(np.uint32))
        d_hits, d_off = _device(part, gpu)
        r1, r2 = _reads(part, gpu)
        cut = None
        if aln is not None:
            pos, nm, op_off, ops = aln[:4]
            w0, w1 = int(op_off[2 * h0]), int(op_off[2 * h1])
            cut = _aln_device((pos[2 * h0:2 * h1], nm[2 * h0:2 * h1], op_off[2 * h0:2 * h1 + 1] - op_off[2 * h0], ops[w0:w1]), gpu)
        w.write(d_hits, d_off, seqs=(r1, r2) if paired else r1, alignments=cut)
    w.close()
    return f.getvalue(), x.getvalue()


@pytest.mark.parametrize("name", ["pe_indel", "se_indel", "edges_pe", "indels_pe", "homopolymers", "long", "power_of_two"])
def test_writers_write_the_alignment(gpu, tmp_path, name):
    """"sam", "sam.gz", "bam" and the sorted "bam" with its index: byte-equal (the compressed ones inflated) to _sam_text(alignments=),
    sam_to_bam of it and write_bam(sort="coordinate", alignments=); the index is build_bai of the device's own file; oriented and
    not; a small chunk_bytes and three batches change nothing"""
    from sailfish_amd import samfile
    k = 8 if name == "indels_pe" else 3
    case, aln = corpus.writable(name, k)
    names, ref_len, seqs = corpus.sam_inputs(case)
    for oriented in (False, True):
        text = samfile._sam_text(names, ref_len, case["hits"], case["off"], None, seqs, oriented=oriented, alignments=aln)
        bam = samfile.sam_to_bam(text)
        assert _written(case, aln, gpu, "sam", oriented)[0] == text
        assert gzip.decompress(_written(case, aln, gpu, "sam.gz", oriented)[0]) == text
        assert gzip.decompress(_written(case, aln, gpu, "bam", oriented)[0]) == bam
        path = str(tmp_path / ("sorted%d.bam" % oriented))
        samfile.write_bam(path, names, ref_len, case["hits"], case["off"], seqs=seqs, oriented=oriented, sort="coordinate", alignments=aln)
        got, bai = _written(case, aln, gpu, "bam", oriented, sort="coordinate")
        assert gzip.decompress(got) == gzip.decompress(open(path, "rb").read())
        assert bai == samfile.build_bai(got) and len(bai) > 8
    longest = max(len(l) for l in text.split(b"\n")) + 1
    chunk = max(4096, 2 * longest + 64)                               # (a unit, the two lines of a pair, fits)
    R = len(case["r1"])
    for fmt, want in (("sam", text), ("bam", bam)):
        small = _written(case, aln, gpu, fmt, True, chunk_bytes=chunk, cuts=[R // 3, R // 3 + 1] if R > 3 else None)[0]
        assert (small if fmt == "sam" else gzip.decompress(small)) == want, fmt
    # without an alignment the writer writes what it wrote before the keyword existed: the statement without one
    if name != "edges_pe":                                            # (its hand-made records hold some that only the band can place)
        plain = samfile._sam_text(names, ref_len, case["hits"], case["off"], None, seqs, oriented=True)
        assert _written(case, None, gpu, "sam", True)[0] == plain and plain != text
        assert gzip.decompress(_written(case, None, gpu, "bam", True)[0]) == samfile.sam_to_bam(plain)


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_without_an_alignment_the_existing_write_corpora_are_unchanged(gpu, paired):
    """write(alignments=None), said aloud, on the writers' own corpora: the random SAM corpus (tests/samwrite_corpus.py) as "sam" and
    "sam.gz", the random BAM corpus (tests/bamwrite_corpus.py) as "bam" -- the bytes those corpora expect, as their own tests do"""
    import bamwrite_corpus as BW
    import samwrite_corpus as SW
    from sailfish_amd import samfile
    from test_gpu_samwrite import _device_seqs, _t
    for case, fmts in ((SW.random_case(1, paired), ("sam", "sam.gz")), (BW.case(paired, n_reads=300, seed=2), ("bam",))):
        want = samfile.sam_header(case["names"], case["ref_len"]) + SW.expected(case)
        for fmt in fmts:
            f = io.BytesIO()
            w = samfile.SamDeviceWriter(f, case["names"], case["ref_len"], paired, format=fmt)
            w.write(_t(case["hits"].view(np.uint8).reshape(-1), gpu), _t(case["offsets"], gpu), read_names=case["read_names"],
                    seqs=_device_seqs(case["seqs"], paired, gpu), alignments=None)
            w.close()
            got = f.getvalue() if fmt == "sam" else gzip.decompress(f.getvalue())
            assert got == (samfile.sam_to_bam(want) if fmt == "bam" else want), fmt


def test_a_cigar_of_40_operations_across_a_tile_boundary(gpu):
    """a mate of 21 stretches of 12 bases with a base deleted or inserted between them (about 40 operations): with enough reads in front
    of it its CIGAR lies across byte 4096 of the batch's text, where two blocks each write their part of it"""
    from sailfish_amd import hits as H
    from sailfish_amd import samfile
    rng = np.random.default_rng(12)
    t = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 1200))
    parts, x = [], 300
    for i in range(21):
        parts.append(t[x:x + 12]); x += 12
        if i % 2 == 0:
            x += 1                                                    # a transcript base skipped
        else:
            parts.append(bytes([{65: 67, 67: 71, 71: 84, 84: 65}[t[x]]]))      # a read base more, unlike the next transcript base
    special = b"".join(parts)
    names, ref_len = [b"t0"], np.array([len(t)], np.uint32)
    sp = H.align_hits_host([t], np.array([(0, 300, 0, 0, len(special), 0, 1, 0, 0, 0)], dtype=H.HIT_DTYPE), [0, 1], [special], None, 3)
    for last_len in range(60, 420):                                   # (reads that match everywhere: <len>M at pos, written here by hand)
        lens = [240] * 14 + [last_len]
        reads = [t[20 * i:20 * i + n] for i, n in enumerate(lens)] + [special]
        recs = np.array([(0, 20 * i, 0, 0, n, 0, 1, 0, 0, 0) for i, n in enumerate(lens)] + [(0, 300, 0, 0, len(special), 0, 1, 0, 0, 0)], dtype=H.HIT_DTYPE)
        off = np.arange(len(reads) + 1, dtype=np.uint32)
        pos = np.array([v for i in range(len(lens)) for v in (20 * i, 0)] + [int(sp[0][0]), 0], np.int32)
        n_ops = np.array([v for _ in lens for v in (1, 0)] + [len(sp[3]), 0], np.uint64)
        ops = np.concatenate([np.array([n << 4 for n in lens], np.uint32), sp[3]])
        aln = (pos, np.zeros(len(pos), np.uint32), np.concatenate([[0], np.cumsum(n_ops)]).astype(np.uint64), ops)
        text = samfile._sam_text(names, ref_len, recs, off, None, reads, alignments=aln)
        body = text[len(samfile.sam_header(names, ref_len)):]
        last = body.rstrip(b"\n").rfind(b"\n") + 1
        cigar = body[last:].split(b"\t")[5]
        a = last + body[last:].index(b"\t" + cigar + b"\t") + 1
        if a + 20 < 4096 < a + len(cigar) - 20:
            break
    else:
        pytest.fail("no length of the read in front puts the CIGAR across the boundary")
    aln = H.align_hits_host([t], recs, off, reads, None, 3)
    assert np.array_equal(aln[0], pos) and np.array_equal(aln[3], ops)
    assert 38 <= int(np.diff(aln[2])[-2]) <= 44 and cigar.count(b"D") >= 8 and cigar.count(b"I") >= 8, cigar
    case = dict(seqs=[t], r1=reads, r2=None, hits=recs, off=off)
    assert _written(case, aln, gpu, "sam")[0] == text
    assert gzip.decompress(_written(case, aln, gpu, "bam")[0]) == samfile.sam_to_bam(text)
    idx = _index(case, gpu)
    pos, nm, op_off, ops, st = H.align_hits(idx, recs, off, reads, max_indel=3)
    _same((*_numpy(pos, nm, op_off, ops), st), aln, "40 operations")
    idx.close()


def test_an_unalignable_slot_fails_the_batch_before_a_byte_is_written(gpu):
    """kind 1, the lowest (read, record) first, in every format; the file holds its header and nothing else"""
    from sailfish_amd import samfile
    for name in ("edges_pe", "edges_se"):
        case = corpus.cases()[name]
        aln = corpus.expected(name, 3)
        n_ops = np.diff(aln[2].astype(np.int64))
        bad = [(r, i - int(case["off"][r])) for r in range(len(case["off"]) - 1) for i in range(case["off"][r], case["off"][r + 1])
               if any(n_ops[2 * i + j] == 0 for j in range(2 if case["hits"][i]["mate_status"] == 3 else 1))]
        names, ref_len, _ = corpus.sam_inputs(case)
        paired = corpus.is_paired(case)
        d_hits, d_off = _device(case, gpu)
        r1, r2 = _reads(case, gpu)
        for fmt, sort in (("sam", None), ("bam", None), ("bam", "coordinate")):
            f = io.BytesIO()
            w = samfile.SamDeviceWriter(f, names, ref_len, paired, format=fmt, sort=sort, index=False)
            with pytest.raises(ValueError, match="read %d, record %d: the read has no base on the transcript" % bad[0]):
                w.write(d_hits, d_off, seqs=(r1, r2) if paired else r1, alignments=_aln_device(aln, gpu))
            w.close()
            if fmt == "sam":
                assert f.getvalue() == samfile.sam_header(names, ref_len)
            else:
                assert gzip.decompress(f.getvalue()) == samfile.sam_to_bam(samfile.sam_header(names, ref_len, sort))
        with pytest.raises(ValueError, match="slots"):
            w = samfile.SamDeviceWriter(io.BytesIO(), names, ref_len, paired)
            w.write(d_hits, d_off, alignments=_aln_device(corpus.expected("first_look", 3), gpu))


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def _spliced_indel_reads(seed=7, n_reads=500):
    """a spliced synthetic transcriptome (60 random exons, ten genes of four isoforms) with single-end reads of 100 bases from either
    strand, 1 % substitutions, and in every second read one insertion or deletion of 1 - 3 bases"""
    import verify_corpus as VC
    import verifyg_corpus as VG
    rng = np.random.default_rng(seed)
    exons = [bytes(rng.choice(VC.ACGT, rng.integers(40, 221))) for _ in range(60)]
    seqs = []
    for gene in range(10):
        own = exons[6 * gene:6 * gene + 6]
        for _ in range(4):
            seqs.append(b"".join(e for i, e in enumerate(own) if i in (0, 5) or rng.random() < 0.6))
    reads = []
    while len(reads) < n_reads:
        t = seqs[int(rng.integers(0, len(seqs)))]
        if len(t) < 104:
            continue
        p = int(rng.integers(0, len(t) - 103))
        r = t[p:p + 104]
        if len(reads) % 2:
            r = VG.with_indel(rng, r, 1, 3)
        r = VC.with_errors(rng, [r[:100]], 0.01)[0]
        reads.append(r if rng.random() < 0.5 else VC.revcomp(r))
    return ["tx%d" % i for i in range(len(seqs))], seqs, reads


def test_quantify_reads_writes_gapped_mappings(gpu, tmp_path):
    """quantify_reads(write_mappings=, validate_mappings=True, max_indel=3, mappings_gapped=True, mappings_oriented=True) writes the
    statement's file; every mapped line replays to its nm; quant.sf and aux/eq_classes.txt are those of the same call without
    mappings_gapped; quantify_files writes the same file from FASTA files; the sorted BAM and its index follow;
    map_reads(validate={..., "align": True}) leaves align_hits' result; the ValueError combinations"""
    import torch
    import sailfish_amd as sf
    from sailfish_amd import hits as H
    from sailfish_amd import samfile
    names, seqs, reads = _spliced_indel_reads()
    batch = 200
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    ref_len = idx.ref_len.cpu().numpy().view(np.uint32)
    h, o = idx.map_reads(reads, validate=dict(max_indel=3, align=True))
    want = H.align_hits(idx, h, o, reads, max_indel=3)
    assert all(torch.equal(a, b) for a, b in zip(idx.last_alignments, want[:4])) and idx.last_align_stats == want[4] and want[4]["jobs_traced"] > 100
    idx.map_reads(reads, validate=dict(max_indel=3))
    assert idx.last_alignments is None
    with pytest.raises(ValueError, match="align"):
        idx.map_reads(reads, validate=dict(align=True))
    body, total, gapped_lines = [], dict.fromkeys(H.ALIGNG_STATS, 0), 0
    for a in range(0, len(reads), batch):
        part = reads[a:a + batch]
        bh, bo = sf.mapper.hits_to_numpy(*idx.map_reads(part))
        fh, fo, _, _ = H.verify_hits_gapped_host(seqs, bh, bo, part, None, 900, False, 3)
        aln = H.align_hits_host(seqs, fh, fo, part, None, 3)
        case = dict(seqs=seqs, r1=part, r2=None, hits=fh, off=fo)
        re = corpus.replay(case, aln)
        assert np.array_equal(re[::2, 0], aln[1][::2].astype(np.int64)) and (re[::2, 1] == 100).all() and not np.diff(aln[2].astype(np.int64))[1::2].any()
        text = samfile._sam_text(names, ref_len, fh, fo, [b"r%d" % (a + i) for i in range(len(part))], part, oriented=True, alignments=aln)
        body.append(text[len(samfile.sam_header(names, ref_len)):])
        gapped_lines += int(((aln[3] & 15) != H.CIGAR_M).sum())
        for key, v in aln[4].items():
            total[key] = max(total[key], v) if key == "scratch_bytes" else total[key] + v
    idx.close()
    assert gapped_lines >= 50
    log = []
    sopt = lambda: sf.SailfishOpts(dumpEq=True, jointLog=lambda lvl, msg: log.append(msg))
    kw = dict(batch_reads=batch, device=gpu, cmd_options={"libType": "U"}, validate_mappings=True, max_indel=3, mappings_oriented=True)
    rc, exp = sf.mapper.quantify_reads(names, seqs, reads, None, "U", str(tmp_path / "gapped"), sopt(), write_mappings=str(tmp_path / "gapped.sam"),
                                       mappings_gapped=True, **kw)
    assert rc == 0 and exp.align_stats == total
    line = [m for m in log if m.startswith("gapped mappings")]
    assert len(line) == 1 and f"{total['jobs_traced']} of {total['jobs']} mates traced" in line[0] and f"{total['unalignable']} mates unalignable" in line[0]
    assert (tmp_path / "gapped.sam").read_bytes() == samfile.sam_header(names, ref_len) + b"".join(body)
    rc, exp0 = sf.mapper.quantify_reads(names, seqs, reads, None, "U", str(tmp_path / "plain"), sopt(), write_mappings=str(tmp_path / "plain.sam"), **kw)
    assert rc == 0 and exp0.align_stats is None and exp0.verify_stats == exp.verify_stats
    for rel in ("quant.sf", os.path.join("aux", "eq_classes.txt")):
        assert (tmp_path / "gapped" / rel).read_bytes() == (tmp_path / "plain" / rel).read_bytes(), rel
    plain = (tmp_path / "plain.sam").read_bytes()
    assert plain != (tmp_path / "gapped.sam").read_bytes() and plain.count(b"\n") == (tmp_path / "gapped.sam").read_bytes().count(b"\n")
    # from the files on: the same reads as FASTA records named r<index> give the same file
    (tmp_path / "tx.fa").write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in zip(names, seqs)))
    (tmp_path / "reads.fa").write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    rc, expf = sf.mapper.quantify_files(str(tmp_path / "tx.fa"), str(tmp_path / "reads.fa"), None, "U", str(tmp_path / "files"), sopt(),
                                        write_mappings=str(tmp_path / "files.sam"), mappings_gapped=True, **kw)
    assert rc == 0 and expf.align_stats == total and (tmp_path / "files.sam").read_bytes() == (tmp_path / "gapped.sam").read_bytes()
    # the sorted BAM of the same run: the statement's records, sorted, with the index of the device's own file
    rc, _ = sf.mapper.quantify_reads(names, seqs, reads, None, "U", str(tmp_path / "sorted"), sopt(), write_mappings=str(tmp_path / "gapped.bam"),
                                     mappings_format="bam", mappings_sorted=True, mappings_gapped=True, **kw)
    assert rc == 0
    got = (tmp_path / "gapped.bam").read_bytes()
    unsorted = samfile.sam_to_bam(samfile.sam_header(names, ref_len) + b"".join(body))
    assert gzip.decompress(got) == samfile.sort_bam_stream(unsorted)
    assert (tmp_path / "gapped.bam.bai").read_bytes() == samfile.build_bai(got)
    for bad in (dict(validate_mappings=True, max_indel=3), dict(write_mappings=str(tmp_path / "x.sam"), max_indel=3),
                dict(write_mappings=str(tmp_path / "x.sam"), validate_mappings=True, max_indel=0)):
        with pytest.raises(ValueError, match="mappings_gapped"):
            sf.mapper.quantify_reads(names, seqs, reads, None, "U", str(tmp_path / "bad"), mappings_gapped=True, device=gpu, **bad)
    assert not (tmp_path / "x.sam").exists()
