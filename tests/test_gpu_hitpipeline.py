"""What the mappings pipeline shares: the slot passes' host driver and batch struct (csrc/hitgroup.h: HitSlotPass,
HitBatchDev, k_hits_rec_read) at the edges of their grids, against hits.align_hits_host / md_tags_host; and the run object behind
mapper.quantify_reads and quantify_files (mapper._MappingsRun): the two drivers write the same files and leave the same counters,
and both give the index back when a batch fails."""
import numpy as np
import pytest

import verify_corpus as VC
import verifyg_corpus as VG
from test_gpu_aligng import _device, _index, _reads
from test_gpu_aligng import _numpy as _aln_numpy
from test_gpu_aligng import _same as _aln_same
from test_gpu_mdtag import _numpy as _md_numpy
from test_gpu_mdtag import _same as _md_same

pytestmark = pytest.mark.gpu


def _one_record_a_read(n):
    """n single-end reads of 40 .. 42 bases on two short transcripts, either strand, one record each; every second read carries
    one substitution, the others match throughout.  Slot 2 h + 1 is never a job."""
    from sailfish_amd import hits as H
    rng = np.random.default_rng(5)
    seqs = [bytes(rng.choice(VC.ACGT, m)) for m in (120, 90)]
    hits, reads = np.zeros(n, H.HIT_DTYPE), []
    for i in range(n):
        tid, length, fwd = i % 2, 40 + i % 3, i % 4 < 2
        p = int(rng.integers(0, len(seqs[tid]) - length + 1))
        r = bytearray(seqs[tid][p:p + length])
        if i % 2:
            r[length // 2] = b"CGTA"[b"ACGT".index(r[length // 2])]
        reads.append(bytes(r) if fwd else VC.revcomp(bytes(r)))
        hits[i]["tid"], hits[i]["pos"], hits[i]["read_len"], hits[i]["fwd"] = tid, p, length, fwd
    return dict(seqs=seqs, r1=reads, r2=None, hits=hits, off=np.arange(n + 1, dtype=np.uint32))


@pytest.mark.parametrize("n", (3, 4, 5, 7, 8, 9))
def test_slot_passes_at_the_edges_of_their_grids(gpu, n):
    """a block holds 16 slots of a 16-lane group (max_indel 3; the tag pass) and 8 of a 32-lane group (max_indel 8): 7, 8, 9 and
    3, 4, 5 records are one slot short of a block, exactly one, and one over.  Every array and the stats are the statement's, and
    the last slot -- never a job here -- has written the end of the offsets"""
    from sailfish_amd import hits as H
    case = _one_record_a_read(n)
    idx = _index(case, gpu)
    d_hits, d_off = _device(case, gpu)
    r1, _ = _reads(case, gpu)
    for k in (3, 8):
        want = H.align_hits_host(case["seqs"], case["hits"], case["off"], case["r1"], None, k)
        assert want[4]["jobs"] == n and 0 < want[4]["jobs_traced"] < n          # all-match and traced mates, both
        *aln, st = H.align_hits(idx, d_hits, d_off, r1, None, max_indel=k)
        got = _aln_numpy(*aln)
        _aln_same((*got, st), want, (n, k))
        assert got[2].shape == (2 * n + 1,) and int(got[2][-1]) == len(want[3]) == int(want[2][-1])
        for alignment, d_aln in ((None, None), (want, tuple(aln))):
            want_md = H.md_tags_host(case["seqs"], case["hits"], case["off"], case["r1"], None, alignment)
            nm, md_off, md, st_md = H.md_tags(idx, d_hits, d_off, r1, None, d_aln)
            got_md = _md_numpy(nm, md_off, md)
            _md_same((*got_md, st_md), want_md, (n, k, alignment is not None))
            assert got_md[1].shape == (2 * n + 1,) and int(got_md[1][-1]) == len(want_md[2]) == int(want_md[1][-1]) and want_md[3]["slots"] == n
    idx.close()


@pytest.fixture(scope="module")
def pairs():
    """20 transcripts; 200 pairs of 2 x 50 bases (mate 2 from the other strand), 1 % substitutions, an indel of 1 - 3 bases in a
    mate of every fifth pair, and every tenth pair random bases -> (names, transcripts, mates 1, mates 2, qualities 1, qualities 2)"""
    rng = np.random.default_rng(11)
    seqs = [bytes(rng.choice(VC.ACGT, int(rng.integers(300, 601)))) for _ in range(20)]
    r1, r2 = [], []
    for i in range(200):
        if i % 10 == 9:
            m1, m2 = (bytes(rng.choice(VC.ACGT, 50)) for _ in range(2))
        else:
            t = seqs[int(rng.integers(0, len(seqs)))]
            flen = int(rng.integers(120, 201))
            p = int(rng.integers(0, len(t) - flen + 1))
            m1, m2 = t[p:p + 54], VC.revcomp(t[p + flen - 54:p + flen])
            if i % 5 == 0:
                m1, m2 = (VG.with_indel(rng, m1, 1, 3), m2) if i % 2 else (m1, VG.with_indel(rng, m2, 1, 3))
            m1, m2 = VC.with_errors(rng, [m1[:50], m2[:50]], 0.01)
        r1.append(m1); r2.append(m2)
    quals = [[bytes(rng.integers(66, 75, len(m)).astype(np.uint8)) for m in mates] for mates in (r1, r2)]
    return ["tx%d" % i for i in range(len(seqs))], seqs, r1, r2, quals[0], quals[1]


def test_the_two_drivers_are_one_pipeline(gpu, tmp_path, pairs):
    """quantify_reads on lists and quantify_files on FASTQ files of the same pairs (records r0, r1, ...), every mapping option on:
    the sorted BAM and its index are the same bytes, and so are quant.sf and the counters of every pass"""
    import sailfish_amd as sf
    names, seqs, r1, r2, q1, q2 = pairs
    (tmp_path / "tx.fa").write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in zip(names, seqs)))
    for path, mates, quals in ((tmp_path / "m_1.fq", r1, q1), (tmp_path / "m_2.fq", r2, q2)):
        path.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, m, q) for i, (m, q) in enumerate(zip(mates, quals))))
    kw = lambda tag: dict(batch_reads=64, device=gpu, cmd_options={"libType": "IU"}, write_mappings=str(tmp_path / (tag + ".bam")), mappings_format="bam",
                          mappings_oriented=True, mappings_sorted=True, validate_mappings=True, max_indel=3, mappings_gapped=True, mappings_tags=True,
                          write_unmapped=(str(tmp_path / (tag + "_u1.fq")), str(tmp_path / (tag + "_u2.fq"))))
    rc, a = sf.mapper.quantify_reads(names, seqs, r1, r2, "IU", str(tmp_path / "lists"), sf.SailfishOpts(), quals1=q1, quals2=q2, **kw("lists"))
    assert rc == 0
    rc, b = sf.mapper.quantify_files(str(tmp_path / "tx.fa"), str(tmp_path / "m_1.fq"), str(tmp_path / "m_2.fq"), "IU", str(tmp_path / "files"), sf.SailfishOpts(),
                                     **kw("files"))
    assert rc == 0
    bam = (tmp_path / "lists.bam").read_bytes()
    assert len(bam) > 1000 and bam == (tmp_path / "files.bam").read_bytes()
    assert (tmp_path / "lists.bam.bai").read_bytes() == (tmp_path / "files.bam.bai").read_bytes()
    assert a.verify_stats == b.verify_stats and a.align_stats == b.align_stats and a.tag_stats == b.tag_stats
    assert a.verify_stats["records_out"] > 100 and a.verify_stats["rescued"] > 0 and a.align_stats["jobs_traced"] > 0 and a.tag_stats["slots"] > 200
    assert a.unmapped_stats["reads"] == b.unmapped_stats["reads"] == 200 and a.unmapped_stats["unmapped"] == b.unmapped_stats["unmapped"] >= 20
    assert (tmp_path / "lists" / "quant.sf").read_bytes() == (tmp_path / "files" / "quant.sf").read_bytes()


@pytest.mark.parametrize("driver", ("quantify_reads", "quantify_files"))
def test_the_index_is_released_when_a_batch_fails(gpu, tmp_path, monkeypatch, pairs, driver):
    """quant.quantify raises after it has taken one batch: the driver passes the exception on, and the QuasiIndex it built has
    given its handle back"""
    import sailfish_amd as sf
    names, seqs, r1, r2, _, _ = pairs
    made = []
    init = sf.mapper.QuasiIndex.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        made.append(self)

    def fails(names_, ref_len, batches, *a, **k):
        hits, offsets = next(iter(batches))
        assert offsets.numel() == 65 and made[0]._h.value
        raise RuntimeError("the batch failed")
    monkeypatch.setattr(sf.mapper.QuasiIndex, "__init__", spy)
    monkeypatch.setattr(sf.quant, "quantify", fails)
    kw = dict(batch_reads=64, device=gpu, write_mappings=str(tmp_path / "m.sam"))
    with pytest.raises(RuntimeError, match="the batch failed"):
        if driver == "quantify_reads":
            sf.mapper.quantify_reads(names, seqs, r1, r2, "IU", str(tmp_path / "out"), **kw)
        else:
            (tmp_path / "tx.fa").write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in zip(names, seqs)))
            for path, mates in ((tmp_path / "m_1.fa", r1), (tmp_path / "m_2.fa", r2)):
                path.write_bytes(b"".join(b">r%d\n%s\n" % (i, m) for i, m in enumerate(mates)))
            sf.mapper.quantify_files(str(tmp_path / "tx.fa"), str(tmp_path / "m_1.fa"), str(tmp_path / "m_2.fa"), "IU", str(tmp_path / "out"), **kw)
    assert len(made) == 1 and not made[0]._h.value
