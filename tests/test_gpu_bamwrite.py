"""The mapper's alignments written compressed from the device: samfile.SamDeviceWriter(format="sam.gz" / "bam") and mappings_format=
of mapper.quantify_files (sfgpu_sam_write_bgzf: the chunks of samtext_write.hip -- SAM lines, or the BAM records of bamwfmt.h --
handed to the BGZF encoder of bgzf_write.hip on the device).  The file must inflate -- under gzip, which knows nothing of this
project -- to samfile._sam_text's bytes resp. to sam_to_bam of them, be BGZF member by member, and read back through the project's
own readers."""
import gzip
import io

import numpy as np
import pytest
import torch

import bamwrite_corpus as bcorpus
import samwrite_corpus as corpus
from test_bgzw_cpu import members
from test_gpu_samwrite import LONG, _batches, _device_seqs, _first_difference, _sample, _t

pytestmark = pytest.mark.gpu


def _written(case, fmt, gpu, cuts, chunk_bytes=0):
    """the case through SamDeviceWriter in the batches `cuts` -> (file bytes, stats)"""
    from sailfish_amd import samfile
    out = io.BytesIO()
    w = samfile.SamDeviceWriter(out, case["names"], case["ref_len"], case["paired"], chunk_bytes=chunk_bytes, format=fmt)
    for h, o, q, s in _batches(case, cuts):
        w.write(_t(h.view(np.uint8).reshape(-1), gpu), _t(o, gpu), read_names=q, seqs=_device_seqs(s, case["paired"], gpu))
    w.close()
    return out.getvalue(), w.stats


def _want(case):
    from sailfish_amd import samfile
    n = len(case["offsets"]) - 1
    seqs = case["seqs"] if case["seqs"] is not None or not case["paired"] else [(b"*", b"*")] * n
    return samfile._sam_text(case["names"], case["ref_len"], case["hits"], case["offsets"], case["read_names"], seqs)


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_sam_gz_inflates_to_sam_text(gpu, paired):
    """corner and random corpus (SEQs of 9 000 and 5 000 bases: lines over several tiles) in two batches, with and without read
    names, with and without bases; the default format still writes the plain text"""
    for case in (corpus.corner(paired, LONG), corpus.random_case(2, paired, long_seqs=LONG)):
        n = len(case["offsets"]) - 1
        for v in corpus.variants(case):
            want = _want(v)
            got, stats = _written(v, "sam.gz", gpu, [0, n // 3, n], chunk_bytes=30000)
            ms = members(got)                              # BGZF: headers, BSIZE walk, one final block each, CRC-32, ISIZE, EOF member
            text = gzip.decompress(got)
            assert text == want, _first_difference(text, want)
            assert stats["bytes_out"] == len(got) and stats["members"] == len(ms) - 1 and stats["header_bytes"] + stats["bytes"] == len(want)
            assert stats["chunks"] >= 2 and len(got) < len(want)                # every batch is chunked on its own
        plain, _ = _written(case, "sam", gpu, [0, n // 3, n])
        assert plain == _want(case)
        got, _ = _written(case, "sam.gz", gpu, [0, n])     # the library's chunk size
        assert gzip.decompress(got) == _want(case)


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_bam_and_sam_gz_over_the_bam_corpora(gpu, paired):
    """the corner corpus of csrc/bamwfmt.h (SEQs of 1, 9 000, 5 000 and 65 535 bases, names of 1 and 254 bytes, a bin at every level)
    and a random one, in two batches, with and without read names, with and without bases: "bam" inflates to sam_to_bam of the
    text byte for byte -- magic, header text and reference list included --, "sam.gz" to the text"""
    from sailfish_amd import samfile
    for case in (bcorpus.corner(paired, LONG), bcorpus.case(paired, n_reads=300, seed=2)):
        n = len(case["offsets"]) - 1
        for v in corpus.variants(case):
            text = _want(v)
            want = samfile.sam_to_bam(text)
            got, stats = _written(v, "bam", gpu, [0, n // 3, n], chunk_bytes=200000)
            ms = members(got)
            data = gzip.decompress(got)
            assert data == want, _first_difference(data, want)
            assert stats["bytes_out"] == len(got) and stats["members"] == len(ms) - 1 and stats["header_bytes"] + stats["bytes"] == len(want)
            assert stats["lines"] == text.count(b"\n") - text.count(b"\n@") - 1 and stats["chunks"] >= 2
            packed, _ = _written(v, "sam.gz", gpu, [0, n // 3, n], chunk_bytes=200000)
            assert gzip.decompress(packed) == text
        got, _ = _written(case, "bam", gpu, [0, n])        # the library's chunk size
        assert gzip.decompress(got) == samfile.sam_to_bam(_want(case))


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_what_bam_cannot_say(gpu, paired):
    """every failing batch of the corpus raises ValueError naming the (read, record) and kind the CPU statement names
    (tests/test_bamwrite_cpu.py checks the corpus against it), counted over the batches, and nothing of it reaches the file; the
    same batch is no error for "sam.gz" unless SAM cannot say it either"""
    from sailfish_amd import samfile
    ok = bcorpus.case(paired, n_reads=20, seed=5)
    kinds = {**samfile.WRITE_KINDS, **samfile.BAM_WRITE_KINDS}
    for bad, read, record, kind in bcorpus.failing(paired):
        for fmt in ("bam", "sam.gz"):
            out = io.BytesIO()
            w = samfile.SamDeviceWriter(out, ok["names"], ok["ref_len"], paired, format=fmt)
            h, o, q, s = next(_batches(ok, [0, 20]))
            w.write(_t(h.view(np.uint8).reshape(-1), gpu), _t(o, gpu), read_names=q, seqs=_device_seqs(s, paired, gpu))
            h, o, q, s = next(_batches(bad, [0, len(bad["offsets"]) - 1]))
            args = (_t(h.view(np.uint8).reshape(-1), gpu), _t(o, gpu))
            kw = dict(read_names=q, seqs=_device_seqs(s, paired, gpu))
            if fmt == "bam":
                with pytest.raises(ValueError) as e:
                    w.write(*args, **kw)
                assert str(e.value) == f"read {20 + read}, record {record}: {kinds[kind]}"
            elif _sam_can_say(bad):                        # SAM has no such rule: the batch's lines follow the first batch's
                w.write(*args, **kw)
                w.close()
                head = samfile.sam_header(ok["names"], ok["ref_len"])
                assert _want(bad).startswith(head) and gzip.decompress(out.getvalue()) == _want(ok) + _want(bad)[len(head):]
            w.close()
            if fmt == "bam":
                assert gzip.decompress(out.getvalue()) == samfile.sam_to_bam(_want(ok))


def _sam_can_say(case):
    try:
        _want(case)
        return True
    except (ValueError, IndexError):
        return False


def test_errors_and_empty_files(gpu):
    """a batch SAM cannot express raises before anything of it reaches the file; a writer without batches writes header + EOF"""
    from sailfish_amd import samfile
    for paired in (True, False):
        bad, read, record, _ = corpus.failing(paired)[0]
        ok = corpus.random_case(3, paired, n_reads=20)
        out = io.BytesIO()
        w = samfile.SamDeviceWriter(out, ok["names"], ok["ref_len"], paired, format="sam.gz")
        h, o, q, s = next(_batches(ok, [0, 20]))
        w.write(_t(h.view(np.uint8).reshape(-1), gpu), _t(o, gpu), read_names=q, seqs=_device_seqs(s, paired, gpu))
        with pytest.raises(ValueError, match=rf"^read {20 + read}, record {record}: "):
            w.write(_t(bad["hits"].view(np.uint8).reshape(-1), gpu), _t(bad["offsets"], gpu))
        w.close()
        assert gzip.decompress(out.getvalue()) == _want(ok)
        out = io.BytesIO()
        samfile.SamDeviceWriter(out, ok["names"], ok["ref_len"], paired, format="sam.gz").close()
        assert gzip.decompress(out.getvalue()) == samfile.sam_header(ok["names"], ok["ref_len"]) and len(members(out.getvalue())) == 2
    with pytest.raises(ValueError, match="format"):
        samfile.SamDeviceWriter(io.BytesIO(), ok["names"], ok["ref_len"], True, format="cram")
    out = io.BytesIO()
    samfile.SamDeviceWriter(out, ok["names"], ok["ref_len"], True, format="bam").close()
    assert gzip.decompress(out.getvalue()) == samfile.sam_to_bam(samfile.sam_header(ok["names"], ok["ref_len"])) and len(members(out.getvalue())) == 2


def test_quantify_files_writes_compressed_mappings(gpu, tmp_path):
    """quantify_files(write_mappings=, mappings_format="sam.gz" / "bam"): quant.sf unchanged, the file inflates to the plain writer's
    text resp. to sam_to_bam of it, SamFile takes the "bam" file for BAM, and quantifying from either reproduces NumReads as the
    plain SAM round trip does"""
    import sailfish_amd as sf
    from sailfish_amd import samfile
    names, seqs, r1, r2 = _sample()
    n = 600
    fa = tmp_path / "transcripts.fasta"
    fa.write_bytes(b"".join(b">" + nm.encode() + b"\n" + s + b"\n" for nm, s in zip(names, seqs)))
    paths = []
    for mate, reads in ((1, r1), (2, r2)):
        p = tmp_path / f"reads_{mate}.fastq"
        p.write_bytes(b"".join(b"@frag.%d%slane=3 mate=%d\n" % (i, b"\t" if i % 3 == 0 else b" ", mate) + r + b"\n+\n" + b"I" * len(r) + b"\n"
                               for i, r in enumerate(reads[:n])))
        paths.append(p)
    fopts = dict(batch_reads=250, cmd_options={"libType": "IU"}, device=gpu)
    files = {}
    for fmt in (None, "sam", "sam.gz", "bam"):
        out = tmp_path / f"q_{fmt}"
        kw = {} if fmt is None else dict(write_mappings=str(tmp_path / f"m.{fmt}"), mappings_format=fmt)
        rc, _ = sf.mapper.quantify_files(fa, *paths, "IU", str(out), sf.SailfishOpts(numFragSamples=5000), **kw, **fopts)
        assert rc == 0
        files[fmt] = (out / "quant.sf").read_bytes()
    assert files["sam"] == files[None] and files["sam.gz"] == files[None] and files["bam"] == files[None]
    plain, packed = (tmp_path / "m.sam").read_bytes(), (tmp_path / "m.sam.gz").read_bytes()
    assert gzip.decompress(packed) == plain and len(members(packed)) >= 4 and len(packed) < len(plain) // 2
    bam = (tmp_path / "m.bam").read_bytes()
    assert gzip.decompress(bam) == samfile.sam_to_bam(plain) and len(members(bam)) >= 4 and len(bam) < len(plain) // 2
    got = {}
    for fmt in ("sam", "sam.gz", "bam"):
        with samfile.SamFile(str(tmp_path / f"m.{fmt}"), gpu, paired=True, names=names) as f:
            assert f.format == ("bam" if fmt == "bam" else "sam")
            got[fmt] = [(h.cpu().numpy().tobytes(), o.cpu().numpy().tobytes()) for h, o in f]
    assert got["sam.gz"] == got["sam"] and got["bam"] == got["sam"] and len(got["sam"]) >= 1
    num_reads = {}
    for fmt in ("sam", "sam.gz", "bam"):
        out = tmp_path / f"back_{fmt}"
        rc, _ = sf.quant.quantify_sam(str(tmp_path / f"m.{fmt}"), "IU", str(out), sf.SailfishOpts(numFragSamples=5000), device=gpu)
        assert rc == 0
        num_reads[fmt] = (out / "quant.sf").read_bytes()
    assert num_reads["sam.gz"] == num_reads["sam"] and num_reads["bam"] == num_reads["sam"]
