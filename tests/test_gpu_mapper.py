"""csrc/mapper.hip at its edges: every case of tests/mapper_corpus.py on the device, record for record and offset for offset against
the restated contract (oracle/mapper_oracle.py), and judged by the corpus' independent brute-force statement (soundness on the
transcripts' bases, completeness for error-free reads); the raw sfgpu_map_reads protocol (capacity, sizing call, empty batch);
batch sizes around the block size.  tests/test_mapper_cpu.py shows that every case reaches the edge it is named for.  Integer
work: every comparison is exact."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import mapper_corpus as MC
from oracle import mapper_oracle as MO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FILL = 0x5A


def _index(c, gpu):
    import sailfish_amd as sf
    return sf.mapper.QuasiIndex(c.transcripts, k=c.k, max_occ=c.max_occ, device=gpu, seeds=c.seeds or 2, seed_len=c.seed_len if c.scan else 0)


def _map(idx, r1, r2=None):
    import sailfish_amd as sf
    return sf.mapper.hits_to_numpy(*idx.map_reads(r1, r2))


def _same(got, want):
    (gh, go), (wh, wo) = got, want
    assert np.array_equal(go, wo), (go[:20], wo[:20])
    assert gh.tobytes() == np.ascontiguousarray(wh).tobytes(), next((i, gh[i], wh[i]) for i in range(len(wh)) if gh[i] != wh[i])


@pytest.mark.parametrize("name", MC.CASE_NAMES)
def test_device_matches_the_contract_and_the_judge(gpu, name):
    c = MC.case(name)
    idx = _index(c, gpu)
    assert (idx.k, idx.M) == (c.k, len(c.transcripts))
    assert idx.n_positions == MC.n_positions(c) and idx.n_kmers == len(MC.table(name))
    for paired in ((True, False) if c.reads2 is not None else (False,)):
        got = _map(idx, c.reads1, c.reads2 if paired else None)
        _same(got, MC.expected_for(name, paired))
        MC.judge(c, *got, paired)                            # the device's own records, by the statement that knows neither kernel nor oracle
        _same(_map(idx, c.reads1, c.reads2 if paired else None), got)        # a reused index: the same records again
    idx.close()


@pytest.mark.parametrize("name,buckets", [("tiny_k8_scan", 256), ("shift0_k8_scan", 65536), ("span_k20_s8", 131072), ("all_short_end", 256), ("all_N_end", 256)])
def test_bucket_count_in_the_index_log_line(gpu, name, buckets):
    """the bucket table's shape is visible only in the log line: 256 buckets at the bottom, 4^8 = 65 536 at k = 8 (shift 0), 2^17
    where the 16-bit prefix of an 8-base seed spans two buckets"""
    from sailfish_amd import _lib
    c = MC.case(name)
    lines = []
    _lib.set_logger(lambda lvl, msg: lines.append(msg))
    try:
        idx = _index(c, gpu)
    finally:
        _lib.set_logger(None)
    line = [x for x in lines if x.startswith("index:")]
    assert len(line) == 1, lines
    m = re.fullmatch(r"index: (\d+) transcripts, (\d+) k-mer positions \((\d+) of A/C/G/T only\), k = (\d+), (\d+) buckets", line[0])
    assert m and [int(x) for x in m.groups()] == [len(c.transcripts), MC.n_positions(c), len(MC.table(name)), c.k, buckets], line
    idx.close()


@pytest.fixture(scope="module")
def batch_pool():
    """reads to fill batches with (the truth-bearing reads of two small cases) and their records, one read at a time"""
    out = {}
    for name in ("k16_S2", "k16_s8"):
        c = MC.case(name)
        h, o = MC.expected(name)
        out[name] = [(c.reads1[r], c.reads2[r], h[o[r]:o[r + 1]]) for r in range(len(c.reads1))]
    return out


@pytest.mark.parametrize("name", ["k16_S2", "k16_s8"])
def test_batch_sizes_around_the_block(gpu, batch_pool, name):
    """n_reads = 0, 1, 255, 256, 257: the lookup and record kernels launch n + 1 lanes, 256 to a block"""
    c = MC.case(name)
    idx = _index(c, gpu)
    pool = batch_pool[name]
    for n in (0, 1, 255, 256, 257):
        pick = [pool[(7 * i + n) % len(pool)] for i in range(n)]
        want_h = np.concatenate([p[2] for p in pick]) if n else np.zeros(0, O.HIT_DTYPE)
        want_o = np.concatenate(([0], np.cumsum([len(p[2]) for p in pick]))).astype(np.uint32)
        _same(_map(idx, [p[0] for p in pick], [p[1] for p in pick]), (want_h, want_o))
    idx.close()


def _raw(idx, r1, r2, capacity, hits=None, n_reads=None, null_reads=False):
    """sfgpu_map_reads as the ABI states it -> (rc, n_hits, offsets with one guard word, the hit buffer's bytes)"""
    from sailfish_amd import _lib
    from sailfish_amd.mapper import pack_sequences
    dev = idx.device
    s1, o1 = (t.to(dev).contiguous() for t in pack_sequences(r1))
    s2 = o2 = None
    if r2 is not None:
        s2, o2 = (t.to(dev).contiguous() for t in pack_sequences(r2))
    if null_reads:
        s1 = o1 = s2 = o2 = None
    n = len(r1) if n_reads is None else n_reads
    off = torch.full((n + 2,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    nh = C.c_uint64(0xDEAD)
    torch.cuda.synchronize(dev)
    rc = idx._L.sfgpu_map_reads(idx._h, _lib.ptr(s1), _lib.ptr(o1), _lib.ptr(s2), _lib.ptr(o2), n, _lib.ptr(hits), capacity, _lib.ptr(off), C.byref(nh),
                                _lib.current_stream_ptr())
    torch.cuda.synchronize(dev)
    off = off.cpu().numpy().view(np.uint32)
    assert off[n + 1] == 0x5A5A5A5A                          # nothing behind offsets[n_reads]
    return rc, nh.value, off[: n + 1], None if hits is None else hits.cpu().numpy().tobytes()


@pytest.mark.parametrize("name", ["capacity_end", "capacity_scan", "pairs_end", "pairs_scan"])
def test_raw_capacity_protocol(gpu, name):
    """capacity exactly n_rec succeeds and writes nothing behind the records; one short is SFGPU_ERR_RANGE with *n_hits and the offsets set
    and no record written; d_hits = NULL with capacity 0 is a sizing call; QuasiIndex.map_reads' retry gives what one sufficient call gives"""
    from sailfish_amd import _lib
    c = MC.case(name)
    wh, wo = MC.expected(name)
    n_rec = len(wh)
    assert n_rec > 1
    idx = _index(c, gpu)
    rc, nh, off, _ = _raw(idx, c.reads1, c.reads2, 0)                                  # the sizing call
    assert rc == _lib.ERR_RANGE and nh == n_rec and np.array_equal(off, wo)
    buf = torch.full(((n_rec + 1) * 24,), FILL, dtype=torch.uint8, device=gpu)
    rc, nh, off, raw = _raw(idx, c.reads1, c.reads2, n_rec - 1, buf)
    assert rc == _lib.ERR_RANGE and nh == n_rec and np.array_equal(off, wo)
    assert raw == bytes([FILL]) * len(raw)                                             # no partial fill
    rc, nh, off, raw = _raw(idx, c.reads1, c.reads2, n_rec, buf)
    assert rc == _lib.OK and nh == n_rec and np.array_equal(off, wo)
    assert raw[: n_rec * 24] == np.ascontiguousarray(wh).tobytes() and raw[n_rec * 24:] == bytes([FILL]) * 24
    gh, go = _map(idx, c.reads1, c.reads2)                                             # (capacity_*: 1200 records > max(4 n, 1024): two calls inside)
    assert gh.tobytes() == raw[: n_rec * 24] and np.array_equal(go, wo)
    idx.close()


@pytest.mark.parametrize("name", ["no_candidate_end", "no_candidate_scan"])
def test_raw_empty_results(gpu, name):
    """no candidate at all: OK with zero records even for a NULL d_hits; n_reads = 0 with null reads: OK and offsets[0] == 0"""
    from sailfish_amd import _lib
    c = MC.case(name)
    idx = _index(c, gpu)
    for r2 in (c.reads2, None):
        rc, nh, off, _ = _raw(idx, c.reads1, r2, 0)
        assert rc == _lib.OK and nh == 0 and not off.any() and len(off) == len(c.reads1) + 1
    rc, nh, off, _ = _raw(idx, [], None, 0, n_reads=0, null_reads=True)
    assert rc == _lib.OK and nh == 0 and off.tolist() == [0]
    buf = torch.full((24,), FILL, dtype=torch.uint8, device=gpu)
    rc, nh, off, raw = _raw(idx, [], None, 1, buf, n_reads=0, null_reads=True)
    assert rc == _lib.OK and nh == 0 and off.tolist() == [0] and raw == bytes([FILL]) * 24
    idx.close()


@pytest.mark.parametrize("name", ["long_mate_end", "long_mate_scan"])
def test_mates_over_65535_bases_get_no_records(gpu, name):
    """the 16-bit length fields: at 65 535 bases read_len, mate_len and frag_len are the true ones; at 65 536 the read has no records
    (k_map_records used to narrow the length: read_len 0 and a fragment 65 536 short), paired and single end, whichever mate it is"""
    c = MC.case(name)
    idx = _index(c, gpu)
    h, o = _map(idx, c.reads1, c.reads2)
    assert np.diff(o.astype(np.int64)).tolist() == [1, 0, 1, 0, 1, 0]
    assert h["frag_len"].tolist() == [65850] * 3 and h["read_len"].tolist() == [65535, 50, 65535] and h["mate_len"].tolist() == [50, 65535, 50]
    assert (h["mate_status"] == 3).all() and h["tid"].tolist() == [0, 0, 0]
    h, o = _map(idx, c.reads1)
    assert np.diff(o.astype(np.int64)).tolist() == [1, 0, 1, 1, 1, 0] and h["read_len"].tolist() == [65535, 50, 50, 65535]
    assert h["pos"].tolist() == [100, 65900, 65900, 100] and h["fwd"].tolist() == [1, 0, 0, 0]
    idx.close()


def test_set_scan_and_set_seeds_switch_one_index(gpu):
    """one index, every mode in turn and back: the mode lives in the handle, not in the table"""
    c = MC.case("k16_S2")
    idx = _index(c, gpu)
    si = MO.build_scan_index(c.transcripts, c.k)
    ei = MO.build_index(c.transcripts, c.k, c.max_occ)
    for seeds, seed_len in ((None, 8), (8, None), (None, 16), (3, None), (2, None)):
        if seed_len:
            idx.set_scan(seed_len)
            want = MO.scan_reads(si, c.reads1, c.reads2, s=seed_len, max_occ=c.max_occ)
        else:
            idx.set_scan(0); idx.set_seeds(seeds)
            want = MO.map_reads(ei, c.reads1, c.reads2, k=c.k, seeds=seeds)
        _same(_map(idx, c.reads1, c.reads2), want)
    _same(_map(idx, c.reads1, c.reads2), MC.expected("k16_S2"))
    idx.close()
