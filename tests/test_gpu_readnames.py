"""Read names kept on the device (sfgpu_reads_parse_host_n / _device_n: the name blob of sailfish_amd/csrc/readtext.hip;
sfgpu_reads_names_match) against the serial run of the same contract header (tests/readnames_harness.cpp), then the file driver
(readfile.ReadFile(names="device"), readfile.mate_names_match) and mapper.quantify_files (write_mappings, check_mate_names)
against the host name list on the bundled sample."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import readnames_corpus as corpus
from test_gpu_readfile import _render, _sample, _texts_for_carry
from test_readfile_cpu import ERR_FORMAT, ERR_RANGE, OK, fastq_text, restate, same, unpack
from test_readnames_cpu import ERR_INVALID, NamesHarness, build_harness, expected_first, round16

pytestmark = pytest.mark.gpu
RES_FIELDS = ("n_reads", "n_bases", "consumed", "n_lines", "error_record", "error_line", "format", "error_kind")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return NamesHarness(build_harness(tmp_path_factory.mktemp("rnh")))


def device_parse(gpu, entry, text, final, max_reads=1 << 40, cap_bases=1 << 40, *, api="n", names=True, cap_names=None, spans=True,
                 misalign=0):
    """one call of sfgpu_reads_parse_<entry>_<api> with qualities -> every output, as bytes and lists"""
    import torch
    from sailfish_amd import _lib
    text = bytes(text)
    n = len(text)
    max_reads, cap_bases = min(max_reads, n + 1), min(cap_bases, n)
    cap_names = max(round16(n), 16) if cap_names is None else cap_names
    bases = torch.zeros(max(cap_bases, 16), dtype=torch.uint8, device=gpu)
    qual = torch.zeros(max(cap_bases, 16), dtype=torch.uint8, device=gpu)
    off = torch.full((max_reads + 1,), -1, dtype=torch.int64, device=gpu)
    span = torch.zeros(2 * max_reads + 2, dtype=torch.int64, device=gpu) if spans else None
    room = torch.full((cap_names + 64,), 0xAA, dtype=torch.uint8, device=gpu)
    blob = room[16 + misalign:16 + misalign + cap_names]
    name_off = torch.full((max_reads + 1,), 77, dtype=torch.int64, device=gpu)
    n_name = C.c_uint64(99)
    res = _lib.ReadsResult()
    L = _lib.lib()
    src = [text, n]
    if entry == "device":
        cap_text = round16(n + 1) + 16
        d_text = torch.zeros(max(cap_text, 16), dtype=torch.uint8, device=gpu)
        d_text[:n] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(gpu)
        src = [_lib.ptr(d_text), n, cap_text]
    args = src + [int(final), max_reads, _lib.ptr(bases), _lib.ptr(qual), cap_bases, _lib.ptr(off), _lib.ptr(span)]
    if api == "n":
        args += [C.c_void_p(blob.data_ptr()) if names else None, cap_names if names else 0, _lib.ptr(name_off) if names else None,
                 C.byref(n_name) if names else None]
    with torch.cuda.device(gpu):
        rc = getattr(L, f"sfgpu_reads_parse_{entry}_{api}")(*args, C.byref(res), _lib.current_stream_ptr())
        torch.cuda.synchronize()
    if rc == ERR_INVALID:                                     # refused before anything was touched
        assert (room == 0xAA).all() and int(off[0]) == -1 and res.n_reads == 0
        return dict(rc=rc)
    sp = span.cpu().numpy().view(np.uint64) if spans else np.zeros(2 * max_reads + 2, np.uint64)
    out = unpack(rc, res, text, bases.cpu().numpy(), off.cpu().numpy(), sp)
    wrote = names and api == "n"
    R, nb = int(res.n_reads), int(n_name.value) if wrote else 0
    o = name_off.cpu().numpy()
    whole = room.cpu().numpy()
    lo = 16 + misalign
    b = whole[lo:lo + nb].tobytes()
    out.update(res={k: int(getattr(res, k)) for k in RES_FIELDS}, bases=bases.cpu().numpy().tobytes(), qual=qual.cpu().numpy().tobytes(),
               off=off.cpu().numpy().tolist(), n_name_bytes=nb, n_name_raw=int(n_name.value), name_off=o[: R + 1].tolist(), raw_name_off=o.tolist(),
               blob=b, blob_names=[b[o[r]:o[r + 1]] for r in range(R)] if rc == OK and wrote else [], pad=whole[lo + nb:lo + round16(nb)].tobytes(),
               # nothing in front of the blob, nothing behind its last 16-byte group
               untouched=bool((whole[:lo] == 0xAA).all() and (whole[lo + round16(nb):] == 0xAA).all()))
    return out


def check(gpu, harness, text, final, max_reads=1 << 40, cap_bases=1 << 40, what=""):
    """both entries against the harness: the _q outputs (same()), the blob, its offsets and n_name_bytes, spans together with the blob"""
    n = len(text)
    want = harness.parse(text, final, min(max_reads, n + 1), min(cap_bases, n))
    ref = restate(text, final, min(max_reads, n + 1), min(cap_bases, n))
    got = None
    for entry in ("host", "device"):
        got = device_parse(gpu, entry, text, final, max_reads, cap_bases)
        same(got, ref, (entry, what))
        assert got["rc"] == want["rc"], (entry, what)
        assert got["n_name_bytes"] == want["n_name_bytes"] and got["blob"] == want["blob"], (entry, what)
        assert got["untouched"], (entry, what)
        if got["rc"] == OK:
            assert got["name_off"] == want["name_off"] and got["blob_names"] == want["names"] == ref["names"], (entry, what)
            assert got["spans"] == want["spans"] and got["names"] == got["blob_names"], (entry, what)      # spans and blob agree
            assert got["pad"] == bytes(len(got["pad"])), (entry, what)
        else:
            assert got["res"]["n_reads"] == 0 and got["res"]["consumed"] == 0 and got["n_name_bytes"] == 0, (entry, what)
    return got


CASES = {label: (text, names) for label, text, names in corpus.gather_cases()}


@pytest.mark.parametrize("label", sorted(CASES))
def test_gather_equals_the_harness(gpu, harness, label):
    """every listed text whole (final and not) and cut short; the whole final text gives the names it was rendered from"""
    text, names = CASES[label]
    got = check(gpu, harness, text, 1, what=label)
    assert got["rc"] == OK and got["blob_names"] == names and not any(b"\r" in nm for nm in got["blob_names"])
    check(gpu, harness, text, 0, what=label)
    for cut in (len(text) - 1, len(text) // 2):
        for final in (0, 1):
            check(gpu, harness, text[:cut], final, what=(label, cut, final))
    if label.startswith("fasta_header_only"):                 # the header-only last line: open when not final, a record when final
        assert len(check(gpu, harness, text, 0)["blob_names"]) == len(names) - 1


def test_texts_without_records(gpu, harness):
    for text in (b"", b"\n", b"\r\n\n", b">", b"@", b">\n>\n>", b">t", b"@r\nAC\n+\nII"):
        for final in (0, 1):
            got = check(gpu, harness, text, final, what=text)
            if got["rc"] == OK:
                assert got["raw_name_off"][0] == 0


def test_cuts_and_errors(gpu, harness):
    text, names = CASES["fastq_mixed"]
    total = sum(len(nm) for nm in names)
    for max_reads, cap in ((5, 1 << 40), (1 << 40, 60), (1, 1 << 40), (7, 100)):
        got = check(gpu, harness, text, 1, max_reads, cap, what=(max_reads, cap))
        assert got["rc"] == OK and 0 < len(got["blob_names"]) < len(names) and got["blob_names"] == names[: len(got["blob_names"])]
    for entry in ("host", "device"):
        assert device_parse(gpu, entry, text, 1, cap_names=round16(total))["blob_names"] == names       # exactly enough
        r = device_parse(gpu, entry, text, 1, cap_names=round16(total) - 16)
        assert r["rc"] == ERR_RANGE and r["res"]["n_reads"] == 0 and r["res"]["consumed"] == 0 and r["n_name_bytes"] == 0
        assert device_parse(gpu, entry, text, 1, misalign=4)["rc"] == ERR_INVALID
        assert device_parse(gpu, entry, text, 1, cap_names=round16(total) + 8)["rc"] == ERR_INVALID
        # a malformed record behind the cut is an error of the call, as for _q
        lines = text.split(b"\n")
        lines[4 * 15 + 2] = b"-"
        bad = b"\n".join(lines)
        r, q = device_parse(gpu, entry, bad, 1, max_reads=3), device_parse(gpu, entry, bad, 1, max_reads=3, api="q")
        assert r["rc"] == q["rc"] == ERR_FORMAT and r["res"] == q["res"] and r["res"]["error_record"] == 15 and r["n_name_bytes"] == 0
        # d_names == NULL: the _q call, byte for byte
        for t, final, max_reads in ((text, 1, 1 << 40), (text, 0, 6), (CASES["fasta_mixed_crlf"][0], 1, 1 << 40)):
            a, b = device_parse(gpu, entry, t, final, max_reads, names=False), device_parse(gpu, entry, t, final, max_reads, api="q")
            for k in ("rc", "res", "bases", "qual", "off", "spans"):
                assert a[k] == b[k], (entry, k)
            assert a["untouched"] and a["n_name_raw"] == 99 and a["raw_name_off"] == b["raw_name_off"]      # nothing of the names was written
            c = device_parse(gpu, entry, t, final, max_reads)                        # ... and with names the _q outputs are the same
            for k in ("rc", "res", "bases", "qual", "off", "spans"):
                assert c[k] == b[k], (entry, k)


def test_name_across_the_staging_boundary(gpu, harness):
    """a host text just over 4 MiB (two staged sub-chunks) with a name lying across the boundary"""
    rng = np.random.default_rng(7)
    rec, _, _ = fastq_text(rng, 1, lens=[1001])
    edge = 4 << 20
    reps = (edge - 4000) // len(rec)
    front = rec * reps
    room = edge - 20 - len(front)                             # one more record, sized so that the next header begins 20 bytes short of the edge
    pad = (room - 7) % 2
    front += b"@f" + b"f" * pad + b"\n" + b"A" * ((room - 7 - pad) // 2) + b"\n+\n" + b"I" * ((room - 7 - pad) // 2) + b"\n"
    assert len(front) == edge - 20
    name = corpus.name_bytes(rng, 60)
    at = len(front) + 1
    assert at < edge < at + len(name)
    text = front + b"@" + name + b" c\nACGT\n+\nIIII\n" + rec * 2
    assert edge < len(text) < edge + (1 << 16)
    got = check(gpu, harness, text, 1)
    assert got["rc"] == OK and got["blob_names"][reps + 1] == name and len(got["blob_names"]) == reps + 4


def _upload(names, gpu):
    import torch
    b, o = corpus.blob_of(names)
    return torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(gpu), torch.from_numpy(o).to(gpu)


def test_match_equals_the_stem_rule(gpu, harness):
    from sailfish_amd import readfile
    seen = set()
    for label, n1, n2 in corpus.match_cases():
        want = expected_first(n1, n2)
        assert harness.match(n1, n2) == want, label
        assert readfile.mate_names_match(_upload(n1, gpu), _upload(n2, gpu)) == want, label
        seen.add((len(n1), want))
    assert {(0, None), (1, None), (200, None), (200, 3), (200, 130), (70, 66)} <= seen
    with pytest.raises(ValueError):
        readfile.mate_names_match(_upload([b"a"], gpu), _upload([b"a", b"b"], gpu))


def _decode(pair):
    b, o = pair
    assert b.is_cuda and o.is_cuda and b.dtype.itemsize == 1 and o.dtype.itemsize == 8
    b, o = b.cpu().numpy().tobytes(), o.cpu().numpy()
    assert o[0] == 0 and o[-1] == len(b)
    return [b[o[r]:o[r + 1]] for r in range(len(o) - 1)]


def _read_all(path, gpu, names, batch, **kw):
    from sailfish_amd import readfile
    got = []
    with readfile.ReadFile(path, gpu, names=names, **kw) as rf:
        while True:
            b, o = rf.read(batch)
            last = rf.last_names
            if o.numel() - 1 == 0:
                assert (_decode(last) if names == "device" else last) == []
                break
            got += _decode(last) if names == "device" else last
            assert names or last == []
        calls = rf.stats["calls"]
    return got, calls


@pytest.mark.parametrize("carrier", ["plain", "bgzf", "gzip_host", "gzip_device"])
def test_read_file_device_names_equal_the_list(gpu, tmp_path, carrier):
    """names="device" decoded = names=True's list = the restatement, with reads that span several parse calls (block_bytes 100)
    and batches smaller than the file; names=False gives no names"""
    from sailfish_amd import gzfile
    texts = list(_texts_for_carry()) + [(CASES["fastq_mixed_crlf"][0], None, CASES["fastq_mixed_crlf"][1])]
    for k, (text, _, names) in enumerate(texts):
        assert restate(text, 1)["names"] == names
        path = tmp_path / f"t{k}"
        kw = {}
        if carrier == "plain":
            path.write_bytes(text)
        elif carrier == "bgzf":
            gzfile.write_bgzf(str(path), text, member_bytes=700)
        else:
            with gzip.open(path, "wb", compresslevel=6) as f:
                f.write(text)
            kw = dict(inflate=carrier[5:])
        for block, batch in ((100, 1 << 40), (100, 7), (1 << 20, 3)):
            dev, calls = _read_all(path, gpu, "device", batch, block_bytes=block, **kw)
            assert dev == names, (carrier, k, block, batch)
            if carrier in ("plain", "gzip_host") and block == 100 and batch > len(names):
                assert calls > 1                              # one read() took several parse calls: blobs concatenated, offsets rebased
            assert _read_all(path, gpu, True, batch, block_bytes=block, **kw)[0] == names
        assert _read_all(path, gpu, False, 1 << 40, **kw)[0] == []


# ---- end to end on the bundled sample ---------------------------------------------------------------------------------------

N_READS, BATCH = 2000, 800


def _records(path):
    ls = path.read_bytes().split(b"\n")
    return [h[1:].split(b" ")[0] for h in ls[0:-1:4]], ls[1::4], ls[3::4]


@pytest.fixture(scope="module")
def sample(gpu, tmp_path_factory):
    """the sample rendered as files, quantified once without mappings, and mapped once for the expected files"""
    import sailfish_amd as sf
    d = tmp_path_factory.mktemp("sample")
    names, seqs, r1, r2 = _sample()
    r1, r2 = r1[:N_READS], r2[:N_READS]
    fa, f1, f2 = _render(d, names, seqs, r1, r2, N_READS)
    opts = dict(batch_reads=BATCH, cmd_options={"libType": "IU"}, device=gpu)
    rc, _ = sf.mapper.quantify_files(fa, f1, f2, "IU", str(d / "plain"), sf.SailfishOpts(numFragSamples=5000), **opts)
    assert rc == 0
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    hits, off = [], [np.zeros(1, np.int64)]
    for a in range(0, N_READS, BATCH):
        h, o = sf.mapper.hits_to_numpy(*idx.map_reads(r1[a:a + BATCH], r2[a:a + BATCH]))
        hits.append(h); off.append(o[1:].astype(np.int64) + off[-1][-1])
    ref_len = idx.ref_len.cpu().numpy()
    idx.close()
    n1, s1, q1 = _records(f1)
    n2, s2, q2 = _records(f2)
    assert len(n1) == N_READS and n1[5] == b"read5/1" and n2[5] == b"read5/2" and s1 == r1
    return dict(dir=d, files=(fa, f1, f2), opts=opts, quant=(d / "plain" / "quant.sf").read_bytes(), names=names, ref_len=ref_len,
                hits=np.concatenate(hits), off=np.concatenate(off).astype(np.uint32), read_names=n1, seqs=list(zip(s1, s2)), quals=list(zip(q1, q2)))


@pytest.mark.parametrize("oriented", [False, True])
@pytest.mark.parametrize("fmt", ["sam", "sam.gz", "bam"])
def test_quantify_files_writes_what_the_list_path_writes(gpu, sample, fmt, oriented):
    import sailfish_amd as sf
    from sailfish_amd import samfile
    d = sample["dir"]
    out, path = d / f"q_{fmt}_{int(oriented)}", d / f"m_{int(oriented)}.{fmt}"
    rc, _ = sf.mapper.quantify_files(*sample["files"], "IU", str(out), sf.SailfishOpts(numFragSamples=5000), write_mappings=str(path),
                                     mappings_format=fmt, mappings_oriented=oriented, **sample["opts"])
    assert rc == 0 and (out / "quant.sf").read_bytes() == sample["quant"]
    want = d / f"want_{int(oriented)}.{fmt}"
    kw = dict(read_names=sample["read_names"], seqs=sample["seqs"], quals=sample["quals"] if oriented else None, oriented=oriented)
    if fmt == "bam":
        samfile.write_bam(str(want), sample["names"], sample["ref_len"], sample["hits"], sample["off"], **kw)
    else:
        samfile.write_sam(str(want), sample["names"], sample["ref_len"], sample["hits"], sample["off"], bgzf=fmt == "sam.gz", **kw)
    got, ref = path.read_bytes(), want.read_bytes()
    if fmt != "sam":
        got, ref = gzip.decompress(got), gzip.decompress(ref)
    assert got == ref and got.count(b"read7/1") >= 2


def test_mate_names_are_checked(gpu, sample):
    import sailfish_amd as sf
    d = sample["dir"]
    fa, f1, f2 = sample["files"]
    run = lambda out, m2, **kw: sf.mapper.quantify_files(fa, f1, m2, "IU", str(d / out), sf.SailfishOpts(numFragSamples=5000), **kw, **sample["opts"])
    rc, _ = run("checked", f2, check_mate_names=True)
    assert rc == 0 and (d / "checked" / "quant.sf").read_bytes() == sample["quant"]
    bad_at = BATCH + 123                                      # in the second batch
    lines = f2.read_bytes().split(b"\n")
    assert lines[4 * bad_at] == b"@read%d/2" % bad_at
    lines[4 * bad_at] = b"@reaD%d/2" % bad_at
    bad = d / "slipped_2.fastq"
    bad.write_bytes(b"\n".join(lines))
    with pytest.raises(ValueError, match=rf"reads_1\.fastq and .*slipped_2\.fastq are out of step at record {bad_at}: 'read{bad_at}/1' against 'reaD{bad_at}/2'"):
        run("slipped", bad, check_mate_names=True)
    rc, _ = run("unchecked", bad)                             # without the keyword the same files quantify as before
    assert rc == 0 and (d / "unchecked" / "quant.sf").read_bytes() == sample["quant"]
    from sailfish_amd import samfile
    rc, _ = run("checked_sam", f2, check_mate_names=True, write_mappings=str(d / "checked.sam"))
    assert rc == 0 and (d / "checked.sam").read_bytes() == samfile._sam_text(sample["names"], sample["ref_len"], sample["hits"], sample["off"],
                                                                               sample["read_names"], sample["seqs"])
