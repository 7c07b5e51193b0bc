"""csrc/merge.hip against the numpy statement of tests/merge_corpus.py, primitive by primitive, in one process: HipEngine's
pack_by_owner / fold_block / export_block / merge_disjoint and the raw sfgpu_eqvec_* / sfgpu_eq_add_block_device calls, at the
edges and on the tie paths that random tables never reach (the corpus says which; tests/test_merge_cpu.py checks that it holds
them).  Integer work: every comparison is byte for byte or array for array."""
import ctypes as C

import numpy as np
import pytest
import torch

import merge_corpus as MC

pytestmark = pytest.mark.gpu

FILL = 0x5A


@pytest.fixture(scope="module")
def eng(gpu):
    from sailfish_amd import distributed as sfd
    return sfd.HipEngine(gpu)


def _dev(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dt).view({np.uint32: np.int32, np.uint64: np.int64}[dt]).copy()).to(dev)


def _vec(t, dev):
    """a corpus table as an EqVec; the hashes go in as they are"""
    from sailfish_amd.eqclass import EqVec
    rp, ids, cnt, hs = t
    return EqVec(_dev(rp, np.uint32, dev), _dev(ids, np.uint32, dev), _dev(cnt, np.uint64, dev), _dev(hs, np.uint64, dev), 0)


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _block(b, dev):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if len(b) else torch.empty(0, dtype=torch.uint8, device=dev)


def _same(vec, want):
    return MC.same_table(vec.to_numpy(), want)


def _lib():
    from sailfish_amd import _lib
    return _lib, _lib.lib()


def _raw_pack(vec, n, dev):
    """sfgpu_eqvec_owner_sizes + sfgpu_eqvec_pack_by_owner -> (sizes, h_block_off, the bytes of the blocks)"""
    _l, L = _lib()
    c = int(vec.size())
    hc = (C.c_uint64 * n)(); hi = (C.c_uint64 * n)(); off = (C.c_uint64 * (n + 1))(*([0x5A5A5A5A5A5A5A5A] * (n + 1)))
    torch.cuda.synchronize(dev)
    st = _l.current_stream_ptr()
    assert L.sfgpu_eqvec_owner_sizes(_l.ptr(vec.rowptr), _l.ptr(vec.hashes), c, n, hc, hi, st) == _l.OK
    sizes = [(int(hc[d]), int(hi[d])) for d in range(n)]
    total = sum(MC.block_bytes(*s) for s in sizes)
    buf = torch.full((total + 8,), FILL, dtype=torch.uint8, device=dev)
    assert L.sfgpu_eqvec_pack_by_owner(_l.ptr(vec.rowptr), _l.ptr(vec.ids), _l.ptr(vec.counts), _l.ptr(vec.hashes), c, n, hc, hi, _l.ptr(buf), off,
                                       st) == _l.OK
    torch.cuda.synchronize(dev)
    raw = _bytes(buf)
    assert raw[total:] == bytes([FILL]) * 8                        # nothing behind the last block is written
    return sizes, [int(x) for x in off], raw[:total]


# ---- pack_by_owner ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.OWNER_CASE_NAMES)
def test_pack_by_owner_matches_numpy(gpu, eng, name):
    t, n = MC.owner_cases()[name]
    want_raw, want_sizes = MC.owner_expected(name)
    vec = _vec(t, gpu)
    buf, sizes = eng.pack_by_owner(vec, n)
    assert sizes == want_sizes
    assert _bytes(buf) == want_raw                                  # the whole buffer, pad bytes included
    sizes, off, raw = _raw_pack(vec, n, gpu)
    assert sizes == want_sizes and off == MC.block_offsets(want_sizes) and raw == want_raw


def test_owner_sizes_and_pack_on_big(gpu, eng):
    """300 000 classes: k_owner_sizes strides its 1024-block grid; the reference is the vectorised numpy statement"""
    _l, L = _lib()
    t, n = MC.big(), MC.BIG_OWNERS
    want_raw, want_sizes = MC.big_expected()
    vec = _vec(t, gpu)
    hc = (C.c_uint64 * n)(); hi = (C.c_uint64 * n)()
    torch.cuda.synchronize(gpu)
    assert L.sfgpu_eqvec_owner_sizes(_l.ptr(vec.rowptr), _l.ptr(vec.hashes), MC.n_classes(t), n, hc, hi, _l.current_stream_ptr()) == _l.OK
    assert [(int(hc[d]), int(hi[d])) for d in range(n)] == want_sizes
    buf, sizes = eng.pack_by_owner(vec, n)
    assert sizes == want_sizes and _bytes(buf) == want_raw


# ---- export_block -------------------------------------------------------------------------------------------------------------
def test_export_block_matches_numpy(gpu, eng):
    tables = dict(real=MC.shards3()["whole"], empty=MC.empty_table(), single_ids=MC.owner_cases()["C257"][0],       # L > C, C = 0, L == C
                  long_label=MC.owner_cases()["pad4_1"][0], wide=MC.owner_cases()["rr7"][0])                       # L > C
    assert MC.n_ids(tables["single_ids"]) == MC.n_classes(tables["single_ids"]) and MC.n_ids(tables["real"]) > MC.n_classes(tables["real"])
    for name, t in tables.items():
        got = _bytes(eng.export_block(_vec(t, gpu)))
        assert len(got) == MC.gather_bytes(MC.n_classes(t), MC.n_ids(t)) and got == MC.export_block(t), name


# ---- fold_block ---------------------------------------------------------------------------------------------------------------
def _fold_parts(eng, packed, w, between=None):
    """every owner folds, in rank order, the block that each shard's pack holds for it -> the owners' finished tables"""
    from sailfish_amd.distributed import block_bytes
    out = []
    for o in range(w):
        b = eng.new_builder(); b.start()
        for buf, sizes in packed:
            start = sum(block_bytes(*sizes[d]) for d in range(o))
            c, l = sizes[o]
            eng.fold_block(b, buf[start:start + block_bytes(c, l)], c, l)
            if between is not None:
                between(b)
        b.finish()
        out.append(b.eqVec().to_numpy()); b.close()
    return out


def test_fold_block_at_each_owner_gives_the_numpy_partition(gpu, eng):
    _l, L = _lib()
    s3 = MC.shards3()
    want_packed, want_parts = MC.numpy_chain(s3["shards"], 3)
    packed = [eng.pack_by_owner(_vec(s, gpu), 3) for s in s3["shards"]]
    for (buf, sizes), (wraw, wsizes) in zip(packed, want_packed):
        assert sizes == wsizes and _bytes(buf) == wraw

    def null_block(b):                                              # a block of 0 classes with a null pointer changes nothing
        assert L.sfgpu_eq_add_block_device(b._h, None, 0, 0, _l.current_stream_ptr()) == _l.OK

    parts = _fold_parts(eng, packed, 3, between=null_block)
    for got, want in zip(parts, want_parts):
        assert MC.same_table(got, want)
    big = [int(c) for p in parts for c in p[2] if c >= 1 << 32]
    assert big == [(1 << 33) + 4]                                   # 2^32 - 1, 2^32 and 5, added exactly


def test_fold_block_reads_a_block_inside_a_larger_buffer(gpu, eng):
    """the driver folds slices of its receive buffer: a block at an offset that is a multiple of 8 and of nothing more"""
    t = MC.shards3()["shards"][1]
    raw, (size,) = MC.pack_by_owner(t, 1)
    alone = eng.new_builder(); alone.start(); eng.fold_block(alone, _block(raw, gpu), *size); alone.finish()
    want = alone.eqVec().to_numpy(); alone.close()
    assert MC.same_table(want, t)
    for lead in (8, 24):
        big = _block(bytes([FILL]) * lead + raw + bytes([FILL]) * 40, gpu)
        view = big[lead:lead + len(raw)]
        assert view.data_ptr() % 8 == 0 and view.data_ptr() % 16 == 8
        b = eng.new_builder(); b.start(); eng.fold_block(b, view, *size); b.finish()
        assert MC.same_table(b.eqVec().to_numpy(), want)
        b.close()
        assert _bytes(big) == bytes([FILL]) * lead + raw + bytes([FILL]) * 40          # the fold reads only


# ---- merge_disjoint -----------------------------------------------------------------------------------------------------------
def _merge(eng, parts, dev):
    blocks, sizes = MC.merge_case(parts)
    return eng.merge_disjoint([_block(b, dev) for b in blocks], sizes)


@pytest.mark.parametrize("name", MC.LAYOUT_NAMES)
def test_merge_disjoint_layouts_give_the_whole_table(gpu, eng, name):
    parts, want = MC.layouts()[name]
    got = _merge(eng, parts, gpu)
    assert got is not None and _same(got, want)
    if MC.n_classes(want) == 0:
        assert got.rowptr.cpu().tolist() == [0] and got.ids.numel() == 0 and got.counts.numel() == 0


@pytest.mark.parametrize("name", MC.MERGE_EQUAL)
def test_merge_disjoint_puts_tied_keys_into_full_hash_order(gpu, eng, name):
    got = _merge(eng, MC.merge_cases()[name], gpu)
    assert got is not None and _same(got, MC.merge_expected(name))


@pytest.mark.parametrize("name", MC.MERGE_NONE)
def test_merge_disjoint_reports_two_labels_under_one_first_id_and_hash(gpu, eng, name):
    assert MC.merge_expected(name) is None
    assert _merge(eng, MC.merge_cases()[name], gpu) is None


def _raw_merge(n_parts, ptrs, nc, ni, dev, n_out=4):
    """sfgpu_eqvec_merge_disjoint on outputs filled with 0x5A -> (status, same_key_twice, the outputs' bytes)"""
    _l, L = _lib()
    outs = [torch.full((8 * n_out,), FILL, dtype=torch.uint8, device=dev) for _ in range(4)]
    tie = C.c_int(0x5A5A5A5A)
    torch.cuda.synchronize(dev)
    rc = L.sfgpu_eqvec_merge_disjoint(ptrs, nc, ni, n_parts, *[_l.ptr(o) for o in outs], C.byref(tie), _l.current_stream_ptr())
    torch.cuda.synchronize(dev)
    return rc, tie.value, [_bytes(o) for o in outs]


def test_merge_disjoint_takes_at_most_64_parts(gpu, eng):
    _l, L = _lib()
    E = MC.empty_table()
    assert _merge(eng, [E] * 64, gpu) is not None
    assert _merge(eng, [MC.shards3()["whole"]] + [E] * 64, gpu) is None             # HipEngine: the caller folds instead
    untouched = [bytes([FILL]) * 32] * 4
    for w in (65, 0):
        ptrs = (C.c_void_p * 65)(); nc = (C.c_uint64 * 65)(); ni = (C.c_uint64 * 65)()
        assert _raw_merge(w, ptrs, nc, ni, gpu) == (_l.ERR_INVALID, 0x5A5A5A5A, untouched)
    ptrs = (C.c_void_p * 2)(); nc = (C.c_uint64 * 2)(0, 1); ni = (C.c_uint64 * 2)(0, 1)      # a null block with a class in it
    assert _raw_merge(2, ptrs, nc, ni, gpu) == (_l.ERR_INVALID, 0x5A5A5A5A, untouched)
    blk = _block(MC.export_block(MC.owner_cases()["C1"][0]), gpu)                              # a class and no room for its ids
    rowptr = torch.full((32,), FILL, dtype=torch.uint8, device=gpu)
    tie = C.c_int(0x5A5A5A5A)
    assert L.sfgpu_eqvec_merge_disjoint((C.c_void_p * 1)(blk.data_ptr()), (C.c_uint64 * 1)(1), (C.c_uint64 * 1)(1), 1, _l.ptr(rowptr), None, None, None,
                                        C.byref(tie), _l.current_stream_ptr()) == _l.ERR_INVALID
    torch.cuda.synchronize(gpu)
    assert tie.value == 0x5A5A5A5A and _bytes(rowptr) == untouched[0]
    rc, tie, outs = _raw_merge(2, ptrs, (C.c_uint64 * 2)(), (C.c_uint64 * 2)(), gpu)          # two empty parts: rowptr = [0], no more
    assert (rc, tie) == (_l.OK, 0) and outs == [bytes(4) + bytes([FILL]) * 28] + untouched[1:]


# ---- the two merge routes -----------------------------------------------------------------------------------------------------
def test_both_merge_routes_give_the_single_builder_table(gpu, eng):
    """the owners' partitions of shards3: merge_disjoint of their export blocks, and every partition packed for one owner and
    folded into one builder (what DistributedQuant._merge_allgather does with them) -- both are the O.EqBuilder table"""
    s3 = MC.shards3()
    _, parts = MC.numpy_chain(s3["shards"], 3)
    vecs = [_vec(p, gpu) for p in parts]
    concat = eng.merge_disjoint([eng.export_block(v) for v in vecs], [(MC.n_classes(p), MC.n_ids(p)) for p in parts])
    assert concat is not None and _same(concat, s3["whole"])
    assert concat.total_reads == int(s3["whole"][2].sum())
    b = eng.new_builder(); b.start()
    for v in vecs:
        buf, (size,) = eng.pack_by_owner(v, 1)
        eng.fold_block(b, buf, *size)
    b.finish()
    folded = b.eqVec()
    assert _same(folded, s3["whole"])
    assert all(torch.equal(x, y) for x, y in zip((concat.rowptr, concat.ids, concat.counts, concat.hashes),
                                                 (folded.rowptr, folded.ids, folded.counts, folded.hashes)))
    b.close()


# ---- what the raw ABI refuses -------------------------------------------------------------------------------------------------
def test_raw_abi_refusals_leave_the_outputs_untouched(gpu, eng):
    _l, L = _lib()
    t, n = MC.owner_cases()["rr3"]
    vec = _vec(t, gpu)
    c = MC.n_classes(t)
    good_sizes = MC.owner_expected("rr3")[1]
    st = _l.current_stream_ptr()
    WORD = 0x5A5A5A5A5A5A5A5A
    filled = lambda k: (C.c_uint64 * k)(*([WORD] * k))
    torch.cuda.synchronize(gpu)
    # sfgpu_eqvec_owner_sizes: n_owners of 0 and 257, null arrays with C > 0
    for n_bad, rp, hs in ((0, vec.rowptr, vec.hashes), (257, vec.rowptr, vec.hashes), (3, None, vec.hashes), (3, vec.rowptr, None)):
        hc, hi = filled(258), filled(258)
        assert L.sfgpu_eqvec_owner_sizes(_l.ptr(rp), _l.ptr(hs), c, n_bad, hc, hi, st) == _l.ERR_INVALID
        assert list(hc) == [WORD] * 258 and list(hi) == [WORD] * 258
    # sfgpu_eqvec_pack_by_owner: the same, and sizes that do not add up to C
    total = MC.block_offsets(good_sizes)[-1]
    short = [(good_sizes[0][0] - 1, good_sizes[0][1] - 1)] + good_sizes[1:]
    arrays = (vec.rowptr, vec.ids, vec.counts, vec.hashes)
    calls = [(0, good_sizes, arrays), (257, good_sizes, arrays), (3, short, arrays)]
    calls += [(3, good_sizes, arrays[:k] + (None,) + arrays[k + 1:]) for k in range(4)]
    for n_bad, sizes, (rp, ids, cnt, hs) in calls:
        hc = (C.c_uint64 * 258)(*[s[0] for s in sizes]); hi = (C.c_uint64 * 258)(*[s[1] for s in sizes])
        off = filled(258)
        buf = torch.full((total + 8,), FILL, dtype=torch.uint8, device=gpu)
        rc = L.sfgpu_eqvec_pack_by_owner(_l.ptr(rp), _l.ptr(ids), _l.ptr(cnt), _l.ptr(hs), c, n_bad, hc, hi, _l.ptr(buf), off, st)
        torch.cuda.synchronize(gpu)
        assert rc == _l.ERR_INVALID, (n_bad, sizes[0])
        assert list(off) == [WORD] * 258 and _bytes(buf) == bytes([FILL]) * (total + 8), (n_bad, sizes[0])
    hc = (C.c_uint64 * 3)(*[s[0] for s in good_sizes]); hi = (C.c_uint64 * 3)(*[s[1] for s in good_sizes]); off = filled(4)
    assert L.sfgpu_eqvec_pack_by_owner(_l.ptr(vec.rowptr), _l.ptr(vec.ids), _l.ptr(vec.counts), _l.ptr(vec.hashes), c, 3, hc, hi, None, off,
                                       st) == _l.ERR_INVALID and list(off) == [WORD] * 4                 # no room for the blocks
    # sfgpu_eqvec_export_block: null arrays with C > 0
    l = MC.n_ids(t)
    for k in range(4):
        rp, ids, cnt, hs = arrays[:k] + (None,) + arrays[k + 1:]
        buf = torch.full((MC.gather_bytes(c, l),), FILL, dtype=torch.uint8, device=gpu)
        assert L.sfgpu_eqvec_export_block(_l.ptr(rp), _l.ptr(ids), _l.ptr(cnt), _l.ptr(hs), c, l, _l.ptr(buf), st) == _l.ERR_INVALID
        torch.cuda.synchronize(gpu)
        assert _bytes(buf) == bytes([FILL]) * MC.gather_bytes(c, l)
    # sfgpu_eq_add_block_device: a null block with a class count, a null handle
    b = eng.new_builder(); b.start()
    assert L.sfgpu_eq_add_block_device(b._h, None, 1, 1, st) == _l.ERR_INVALID
    assert L.sfgpu_eq_add_block_device(None, None, 0, 0, st) == _l.ERR_INVALID
    b.finish()
    assert b.n_classes == 0 and b.total_reads == 0
    b.close()
    # (n_parts of 0 and 65 and a null block of sfgpu_eqvec_merge_disjoint: test_merge_disjoint_takes_at_most_64_parts)
