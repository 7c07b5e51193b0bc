"""The coordinate-sorted BAM file and its BAI index written from the device: samfile.SamDeviceWriter(format="bam", sort="coordinate")
and mappings_sorted= of mapper.quantify_files (csrc/bamsort.hip: the records kept on the device, one stable sort, the gather into
the BGZF encoder, the index kernels).  The file must inflate to the host statement write_bam(sort="coordinate") byte for byte, the
index must be build_bai of the device's own file byte for byte, and fetch through the pair must find what a brute-force scan finds."""
import gzip
import io
import os

import numpy as np
import pytest
import torch

import bamsort_corpus as corpus
from samwrite_corpus import blob
from test_gpu_samwrite import _device_seqs, _first_difference, _sample, _t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    """per case: (case, the host statement's inflated stream, its records), computed once"""
    out = {}
    for name, case in corpus.cases().items():
        stream = corpus.sorted_stream(case)
        out[name] = (case, stream, corpus.records(stream))
    return out


def _device_quals(quals, paired, gpu):
    if quals is None:
        return None
    mates = [[q[m] for q in quals] for m in (0, 1)] if paired else [quals]
    ts = [_t(blob(m, np.int64)[0], gpu) for m in mates]
    return tuple(ts) if paired else ts[0]


def _write(w, case, batches, gpu):
    for b in batches:
        w.write(_t(b["hits"].view(np.uint8).reshape(-1), gpu), _t(b["offsets"], gpu), read_names=b["read_names"],
                seqs=_device_seqs(b["seqs"], case["paired"], gpu), quals=_device_quals(b["quals"], case["paired"], gpu))


def _sorted(case, gpu, target, batches=None, **kw):
    """the case's batches through the sorting writer into `target` (a path or a file object) -> stats"""
    from sailfish_amd import samfile
    w = samfile.SamDeviceWriter(target, case["names"], case["ref_len"], case["paired"], format="bam", oriented=case["oriented"], sort="coordinate", **kw)
    _write(w, case, case["batches"] if batches is None else batches, gpu)
    w.close()
    return w.stats


@pytest.mark.parametrize("name", ["edges", "pairs", "big", "many_refs", "single", "nothing"])
def test_sorted_file_and_index(gpu, cases, tmp_path, name):
    """the device file inflates to write_bam(sort="coordinate") inflated; the device index is build_bai of the device file; fetch
    through the device pair equals brute force over the region grid"""
    from sailfish_amd import samfile
    case, want, recs = cases[name]
    path = str(tmp_path / "sorted.bam")
    stats = _sorted(case, gpu, path)
    blob_ = open(path, "rb").read()
    got = gzip.decompress(blob_)
    assert got == want, _first_difference(got, want)
    assert samfile.header_sort_order(path) == "coordinate"
    bai = open(path + ".bai", "rb").read()
    want_bai = samfile.build_bai(blob_)
    assert bai == want_bai, _first_difference(bai, want_bai)
    assert stats["records"] == len(recs) and stats["no_coor"] == sum(r[0] < 0 for r in recs) and stats["index_bytes"] == len(bai)
    assert stats["bytes_out"] == len(blob_) and stats["state_bytes"] >= sum(len(r[3]) + 20 for r in recs)      # the records and 20 B each, at least
    assert all(k in stats for k in ("ms_sort", "ms_gather", "ms_index", "ms_encode"))
    members, _, _ = samfile._bgzf_members(blob_)
    head = samfile._bam_header(got)[2]
    first = -(-head // 32768)
    assert all(m[2] == 32768 for m in members[first:-2]) and members[first][1] == head if recs else len(members) == first + 1
    for tid, beg, end in corpus.regions(case):
        assert samfile.fetch(path, tid, beg, end) == corpus.brute_force(recs, tid, beg, end), (tid, beg, end)


def test_pieces_do_not_change_the_file(gpu, cases):
    """chunk_bytes small enough for several pieces (one member each): the file and the index are those of the default"""
    case, want, _ = cases["big"]
    files = []
    for chunk in (0, 40000, 70000):
        f, x = io.BytesIO(), io.BytesIO()
        _sorted(case, gpu, f, chunk_bytes=chunk, index=x)
        files.append((f.getvalue(), x.getvalue()))
    assert gzip.decompress(files[0][0]) == want and len(want) > 4 * 32768
    assert files[1] == files[0] and files[2] == files[0]


@pytest.mark.parametrize("name", ["edges", "pairs"])
def test_collated_reading_gives_the_unsorted_file_s_records(gpu, cases, tmp_path, name):
    """SamFile(sorted.bam, collate="auto") collates (the header says coordinate) and yields, read by read, the records SamFile
    yields from the unsorted file of the same batches: compared as the multiset of the reads' record sets, for the reads are
    numbered by their first lines and those stand elsewhere"""
    from sailfish_amd import samfile
    case, _, _ = cases[name]
    names = [n.decode() for n in case["names"]]
    paths = {s: str(tmp_path / f"{s}.bam") for s in ("sorted", "unsorted")}
    _sorted(case, gpu, paths["sorted"])
    w = samfile.SamDeviceWriter(paths["unsorted"], case["names"], case["ref_len"], case["paired"], format="bam", oriented=case["oriented"])
    _write(w, case, case["batches"], gpu)
    w.close()
    groups = {}
    for s, path in paths.items():
        with samfile.SamFile(path, gpu, paired=case["paired"], names=names, collate="auto") as f:
            assert f.collated == (s == "sorted")
            g = []
            for h, o in f:
                h, o = h.cpu().numpy().view(np.uint8).reshape(-1, 24), o.cpu().numpy().astype(np.int64)
                g += [tuple(sorted(h[a:b].tobytes()[24 * k:24 * k + 24] for k in range(b - a))) for a, b in zip(o[:-1], o[1:])]
        groups[s] = sorted(g)
    assert groups["sorted"] == groups["unsorted"] and len(groups["sorted"]) == sum(len(b["offsets"]) - 1 for b in case["batches"])


def test_a_failing_batch_leaves_the_store_as_it_was(gpu, cases):
    """a batch that breaks a write rule raises as the unsorted writer does, read counted over the batches, and keeps nothing: the
    file and the index are those written without it"""
    from sailfish_amd import samfile
    from samwrite_corpus import rec
    case, want, _ = cases["edges"]
    rng = np.random.default_rng(3)
    bad = corpus._batch(rng, False, [(b"fine", [rec(0, 5, 0, 0, 50, 0, 1, 0, 0)]), (b"nobase", [rec(0, -50, 0, 0, 50, 0, 1, 0, 0)]),
                                     (b"notid", [rec(9, 5, 0, 0, 50, 0, 1, 0, 0)])])
    n0 = len(case["batches"][0]["offsets"]) - 1
    out, x = io.BytesIO(), io.BytesIO()
    w = samfile.SamDeviceWriter(out, case["names"], case["ref_len"], False, format="bam", oriented=True, sort="coordinate", index=x)
    _write(w, case, case["batches"][:1], gpu)
    with pytest.raises(ValueError) as e:
        _write(w, case, [bad], gpu)
    assert str(e.value) == f"read {n0 + 1}, record 0: {samfile.WRITE_KINDS[1]}"
    _write(w, case, case["batches"][1:], gpu)
    w.close()
    assert gzip.decompress(out.getvalue()) == want and x.getvalue() == samfile.build_bai(out.getvalue())
    assert w.stats["reads"] == sum(len(b["offsets"]) - 1 for b in case["batches"])
    with pytest.raises(ValueError, match="closed"):
        _write(w, case, case["batches"][:1], gpu)


def test_index_targets(gpu, cases, tmp_path):
    """index=None: path + ".bai" beside a path, nothing for a file object; index=False: nothing; a path or a file object: there"""
    from sailfish_amd import samfile
    case, want, _ = cases["pairs"]
    p = str(tmp_path / "a.bam")
    _sorted(case, gpu, p, index=False)
    assert not os.path.exists(p + ".bai") and gzip.decompress(open(p, "rb").read()) == want
    f = io.BytesIO()
    stats = _sorted(case, gpu, f)
    assert stats["index_bytes"] == 0 and gzip.decompress(f.getvalue()) == want and f.getvalue() == open(p, "rb").read()
    x = io.BytesIO()
    _sorted(case, gpu, str(tmp_path / "b.bam"), index=x)
    assert x.getvalue() == samfile.build_bai(str(tmp_path / "b.bam")) and not os.path.exists(str(tmp_path / "b.bam.bai")) and not x.closed
    other = str(tmp_path / "elsewhere.bai")
    _sorted(case, gpu, str(tmp_path / "c.bam"), index=other)
    assert open(other, "rb").read() == x.getvalue()


@pytest.mark.parametrize("fmt", ["sam", "sam.gz", "bam"])
def test_unsorted_formats_write_what_they_wrote(gpu, cases, fmt):
    """sort=None, given or left out: the three formats against their host statements, as the writers' own tests compare them"""
    from sailfish_amd import samfile
    case, _, _ = cases["pairs"]
    m = corpus.merged(case)
    text = samfile._sam_text(case["names"], case["ref_len"], m["hits"], m["offsets"], m["read_names"], m["seqs"], quals=m["quals"], oriented=True)
    want = {"sam": text, "sam.gz": text, "bam": samfile.sam_to_bam(text)}[fmt]
    files = []
    for kw in ({}, {"sort": None}):
        out = io.BytesIO()
        w = samfile.SamDeviceWriter(out, case["names"], case["ref_len"], True, format=fmt, oriented=True, **kw)
        _write(w, case, case["batches"], gpu)
        w.close()
        files.append(out.getvalue())
        assert "records" not in w.stats
    assert files[0] == files[1] and (files[0] if fmt == "sam" else gzip.decompress(files[0])) == want


def test_quantify_files_writes_sorted_mappings(gpu, tmp_path):
    """quantify_files(mappings_format="bam", mappings_sorted=True): quant.sf is the run's without the option, the file is the
    unsorted file's records in coordinate order, the index beside it is build_bai of it, and fetch finds what brute force finds"""
    import sailfish_amd as sf
    from sailfish_amd import samfile
    names, seqs, r1, r2 = _sample()
    n = 600
    fa = tmp_path / "transcripts.fasta"
    fa.write_bytes(b"".join(b">" + nm.encode() + b"\n" + s + b"\n" for nm, s in zip(names, seqs)))
    paths = []
    for mate, reads in ((1, r1), (2, r2)):
        p = tmp_path / f"reads_{mate}.fastq"
        p.write_bytes(b"".join(b"@frag.%d mate=%d\n" % (i, mate) + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads[:n])))
        paths.append(p)
    fopts = dict(batch_reads=250, cmd_options={"libType": "IU"}, device=gpu, mappings_format="bam", mappings_oriented=True)
    quant = {}
    for s in (False, True):
        out = tmp_path / f"q{int(s)}"
        rc, _ = sf.mapper.quantify_files(fa, *paths, "IU", str(out), sf.SailfishOpts(numFragSamples=5000), write_mappings=str(tmp_path / f"m{int(s)}.bam"),
                                         mappings_sorted=s, **fopts)
        assert rc == 0
        quant[s] = (out / "quant.sf").read_bytes()
    assert quant[True] == quant[False]
    plain, path = gzip.decompress((tmp_path / "m0.bam").read_bytes()), str(tmp_path / "m1.bam")
    got = gzip.decompress(open(path, "rb").read())
    assert got == samfile.sort_bam_stream(plain) and samfile.header_sort_order(path) == "coordinate"
    assert open(path + ".bai", "rb").read() == samfile.build_bai(path) and not os.path.exists(str(tmp_path / "m0.bam.bai"))
    recs = corpus.records(got)
    assert len(recs) > 1000
    lens = samfile.read_bam_header(path)[1]
    for tid in range(0, len(names), max(1, len(names) // 12)):
        for beg, end in ((0, lens[tid]), (lens[tid] // 2, lens[tid] // 2 + 100), (16383, 16385)):
            assert samfile.fetch(path, tid, beg, end) == corpus.brute_force(recs, tid, beg, end)
