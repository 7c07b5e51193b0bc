"""Per-read hit filtering on the device -- host mirror of the loop bodies of processReadsQuasi
(src/SailfishQuantify.cpp:215-417 paired end, :530-626 single end) and of sailfish::utils::compatibleHit / hitType
(src/SailfishUtils.cpp:157-289): the mapper's hit records go in, the packed transcript-id lists that
EquivalenceClassBuilder.add_batch takes come out (device-resident), plus the fragment-length samples and the
fragment counters of the ReadExperiment."""
import ctypes as C

import numpy as np
import torch

from . import _lib

# one record per hit: sfgpu_hit (include/sfgpu.h), fields of rapmap's QuasiAlignment that the loop reads
HIT_DTYPE = np.dtype([("tid", "<u4"), ("pos", "<i4"), ("mate_pos", "<i4"), ("frag_len", "<u4"), ("read_len", "<u2"),
                      ("mate_len", "<u2"), ("fwd", "u1"), ("mate_fwd", "u1"), ("mate_status", "u1"), ("pad_", "u1")])
assert HIT_DTYPE.itemsize == 24
# one score per record that survives verify_hits: sfgpu_hit_score
SCORE_DTYPE = np.dtype([("mism", "<u2"), ("over", "<u2"), ("mate_mism", "<u2"), ("mate_over", "<u2")])
assert SCORE_DTYPE.itemsize == 8
# ... and one per record that survives verify_hits(max_indel=1 .. 15): sfgpu_hit_gscore
GSCORE_DTYPE = np.dtype([("edits", "<u2"), ("ungapped", "<u2"), ("mate_edits", "<u2"), ("mate_ungapped", "<u2")])
assert GSCORE_DTYPE.itemsize == 8
MAX_INDEL = 15
SINGLE_END, PAIRED_END_LEFT, PAIRED_END_RIGHT, PAIRED_END_PAIRED = 0, 1, 2, 3        # rapmap::utils::MateStatus
SAME, AWAY, TOWARD, NONE = 0, 1, 2, 3                                                # ReadOrientation
SA, AS, S, A, U = 0, 1, 2, 3, 4                                                      # ReadStrandedness

# parseLibraryFormatStringNew's table (src/SailfishUtils.cpp:69-81): name -> (type, orientation, strandedness)
LIBRARY_FORMATS = {"IU": (1, TOWARD, U), "ISF": (1, TOWARD, SA), "ISR": (1, TOWARD, AS), "OU": (1, AWAY, U),
                   "OSF": (1, AWAY, SA), "OSR": (1, AWAY, AS), "MU": (1, SAME, U), "MSF": (1, SAME, S),
                   "MSR": (1, SAME, A), "U": (0, NONE, U), "SF": (0, NONE, S), "SR": (0, NONE, A)}


def format_id(fmt):
    """LibraryFormat::formatID (include/LibraryFormat.hpp:89-98): type | orientation << 1 | strandedness << 3"""
    t, o, s = fmt
    return (int(t) & 0x01) | ((int(o) & 0x3) << 1) | ((int(s) & 0x7) << 3)


def format_from_id(i):
    """LibraryFormat::formatFromID (include/LibraryFormat.hpp:34-85)"""
    return (int(i) & 0x01, (int(i) >> 1) & 0x3, (int(i) >> 3) & 0x7)


MAX_LIB_TYPE_ID = format_id((1, NONE, U))            # LibraryFormat::maxLibTypeID (:25-30)


def format_check(fmt):
    """LibraryFormat::check (src/LibraryFormat.cpp:6-51): is the combination meaningful?"""
    t, o, s = fmt
    if t == 0:                                       # single end: no orientation, no two-strand protocol
        return o == NONE and s not in (SA, AS)
    if o == NONE:
        return False
    if o == SAME:
        return s in (S, A, U)
    return s in (SA, AS, U)                          # AWAY / TOWARD: the mates come from different strands


def format_str(fmt):
    """operator<<(ostream&, LibraryFormat) (src/LibraryFormat.cpp:53-100), the text of the log lines"""
    t, o, s = fmt
    return ("Library format { type:" + ("single end", "paired end")[t] + ", relative orientation:" +
            {TOWARD: "inward", AWAY: "outward", SAME: "matching", NONE: "none"}[o] + ", strandedness:" +
            {SA: "(sense, antisense)", AS: "(antisense, sense)", S: "sense", A: "antisense", U: "unstranded"}[s] + " }")


def filter_hits(hits, hit_offsets, lib_format, sopt=None, *, paired_library=None, allow_orphans=False,
                ignore_lib_compat=False, enforce_lib_compat=False, allow_dovetail=False, max_read_occs=200,
                max_frag_len=1000, fl_counts=None, remaining_fl_ops=0, stats=None, device="cuda"):
    """hits: numpy structured array (HIT_DTYPE) or a uint8 device tensor of the same bytes; hit_offsets: uint32[R+1].
    lib_format: a name of LIBRARY_FORMATS or a (type, orientation, strandedness) triple.
    Returns (ids int32 device tensor, offsets int32 device tensor [R+1], remaining_fl_ops, stats dict); fl_counts
    (int32 device tensor [max_frag_len]) is updated in place when given."""
    dev = torch.device(device)
    if sopt is not None:
        max_read_occs, max_frag_len = sopt.maxReadOccs, sopt.maxFragLen
    fmt = LIBRARY_FORMATS[lib_format.upper()] if isinstance(lib_format, str) else tuple(lib_format)
    if paired_library is None:
        paired_library = fmt[0] == 1
    if isinstance(hits, torch.Tensor):
        d_hits = hits.to(dev).contiguous()
    else:
        h = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        d_hits = torch.from_numpy(h.view(np.uint8).reshape(-1).copy()).to(dev)
    off = hit_offsets
    d_off = off.to(dev).contiguous() if isinstance(off, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(off, np.uint32).view(np.int32).copy()).to(dev)
    R = int(d_off.numel()) - 1
    n_hits = d_hits.numel() // 24
    ids = torch.empty(max(n_hits, 1), dtype=torch.int32, device=dev)
    out_off = torch.empty(R + 1, dtype=torch.int32, device=dev)
    o = _lib.FilterOpts(int(max_read_occs), int(max_frag_len), int(bool(paired_library)), int(not allow_orphans),
                        int(bool(ignore_lib_compat)), int(bool(enforce_lib_compat)), int(bool(allow_dovetail)),
                        _lib.LibFmt(int(fmt[0]), int(fmt[1]), int(fmt[2]), 0))
    st = _lib.FilterStats()
    if stats:
        for k, v in stats.items():
            setattr(st, k, int(v))
    rem = C.c_int64(int(remaining_fl_ops))
    with torch.cuda.device(dev):
        torch.cuda.current_stream().synchronize()
        _lib.check(_lib.lib().sfgpu_filter_hits(_lib.ptr(d_hits), _lib.ptr(d_off), R, C.byref(o), _lib.ptr(ids), _lib.ptr(out_off),
                                                _lib.ptr(fl_counts) if fl_counts is not None else None, C.byref(rem),
                                                C.byref(st), _lib.current_stream_ptr()))
    total = int(out_off[-1].item()) & 0xFFFFFFFF if R >= 0 else 0
    return ids[:total], out_off, int(rem.value), {k: int(getattr(st, k)) for k, _ in _lib.FilterStats._fields_}


def _device_hits(hits, hit_offsets, dev):
    if isinstance(hits, torch.Tensor):
        d_hits = hits.to(dev).contiguous()
    else:
        h = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        d_hits = torch.from_numpy(h.view(np.uint8).reshape(-1).copy()).to(dev)
    off = hit_offsets
    d_off = off.to(dev).contiguous() if isinstance(off, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(off, np.uint32).view(np.int32).copy()).to(dev)
    return d_hits, d_off


_BASE_CODE = np.full(256, 4, np.uint8)
for _i, _b in enumerate(b"ACGT"):
    _BASE_CODE[_b] = _BASE_CODE[_b + 32] = _i
VERIFY_STATS = ("records_in", "records_out", "reads_in", "reads_out", "failed_identity", "dropped_not_best", "sum_mism")
VERIFYG_STATS = ("records_in", "records_out", "reads_in", "reads_out", "failed_identity", "dropped_not_best", "sum_edits", "rescued")


def _max_indel(max_indel):
    k = int(max_indel)
    if k != max_indel or not 0 <= k <= MAX_INDEL:
        raise ValueError(f"max_indel = {max_indel!r} is no integer in 0 .. {MAX_INDEL}")
    return k


def _permille(min_identity):
    p = int(round(float(min_identity) * 1000))
    if not 0 <= p <= 1000:
        raise ValueError(f"min_identity = {min_identity!r} lies outside 0 .. 1")
    return p


def _oriented_codes(read, fwd):
    """a mate's oriented base codes: code(r[j]) forward, 3 - code(r[len - 1 - j]) reverse, 4 staying 4 on either strand"""
    c = _BASE_CODE[np.frombuffer(read, np.uint8)]
    return c if fwd else np.where(c > 3, 4, 3 - c).astype(np.uint8)[::-1]


def _record_jobs(h, r, reads1, reads2):
    """the jobs of record h of read r: (mate's bytes, forward?, pos) each"""
    st = int(h["mate_status"])
    jobs = [(reads2[r] if st == 2 else reads1[r], bool(h["fwd"]), int(h["pos"]))]
    if st == 3:
        jobs.append((reads2[r], bool(h["mate_fwd"]), int(h["mate_pos"])))
    return jobs


def _score4(per_job):
    """a survivor's score: two fields a job, saturating at 65 535, the mate's 0 where the record has one job"""
    flat = [min(v, 65535) for pair in per_job for v in pair] + [0, 0]
    return tuple(flat[:4])


def _select_survivors(hits, off, record, keep_best, stat_names, score_dtype):
    """PASS, BEST, ORDER and the stats of both verification statements.  record(r, i) -> (ok, cost, score tuple, what a survivor adds
    to the stats: a dict) for record i of read r.  -> (hits, offsets uint32[R + 1], scores, stats dict)"""
    keep, scores, out_off = [], [], [0]
    stats = dict.fromkeys(stat_names, 0)
    stats["records_in"] = int(off[-1]) if len(off) else 0
    for r in range(len(off) - 1):
        recs = [(i, *record(r, i)) for i in range(off[r], off[r + 1])]
        passing = [x for x in recs if x[1]]
        stats["failed_identity"] += len(recs) - len(passing)
        if keep_best and passing:
            best = min(x[2] for x in passing)
            stats["dropped_not_best"] += sum(x[2] != best for x in passing)
            passing = [x for x in passing if x[2] == best]
        for i, _, _, score, extra in passing:
            keep.append(i)
            scores.append(score)
            for key, v in extra.items():
                stats[key] += v
        stats["reads_in"] += int(off[r + 1] > off[r])
        stats["reads_out"] += int(bool(passing))
        out_off.append(len(keep))
    stats["records_out"] = len(keep)
    return hits[np.array(keep, np.int64)] if keep else hits[:0], np.array(out_off, np.uint32), np.array(scores, dtype=score_dtype), stats


def verify_hits_host(transcripts, hits, offsets, reads1, reads2, min_identity_permille, keep_best):
    """The statement of hit verification (csrc/verifyfmt.h restated in numpy; what sfgpu_hits_verify is judged by).  transcripts,
    reads1, reads2 (or None): lists of bytes; hits: HIT_DTYPE records in CSR form over the reads (offsets[R + 1]).  A job is one mate
    of one record -- status 0 / 1: mate 1, strand fwd, at pos; 2: mate 2, fwd, pos; 3: both, the second with mate_fwd at mate_pos --
    of len(mate) bases.  Oriented base j is code(r[j]) forward and 3 - code(r[len - 1 - j]) reverse (A C G T in either case 0 .. 3,
    anything else 4 on either strand); at x = pos + j off the transcript it counts in `over`, else it is a mismatch when either code is
    4 or the codes differ.  A job passes iff 1000 (len - over - mism) >= permille len, a record iff all its jobs pass; keep_best keeps,
    of a read's passing records, those of minimum mism + over.  -> (hits, offsets uint32[R + 1], scores SCORE_DTYPE, stats dict);
    ValueError naming the lowest record whose tid is not a transcript."""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    off = np.asarray(offsets).astype(np.int64)
    permille = int(min_identity_permille)
    if not 0 <= permille <= 1000:
        raise ValueError("min_identity_permille lies outside 0 .. 1000")
    bad = np.nonzero(hits["tid"][: off[-1]] >= len(transcripts))[0]
    if len(bad):
        raise ValueError(f"record {int(bad[0])} names transcript >= {len(transcripts)}")
    tcodes = {}

    def count(read, fwd, tid, pos):
        q = _oriented_codes(read, fwd)
        if tid not in tcodes:
            tcodes[tid] = _BASE_CODE[np.frombuffer(transcripts[tid], np.uint8)]
        t = tcodes[tid]
        x = int(pos) + np.arange(len(q), dtype=np.int64)
        on = (x >= 0) & (x < len(t))
        a, b = q[on], t[x[on]]
        return int(((a > 3) | (b > 3) | (a != b)).sum()), int(len(q) - on.sum())

    def record(r, i):
        jobs = _record_jobs(hits[i], r, reads1, reads2)
        counts = [count(rd, f, int(hits[i]["tid"]), p) for rd, f, p in jobs]
        ok = all(1000 * (len(rd) - ov - mm) >= permille * len(rd) for (rd, _, _), (mm, ov) in zip(jobs, counts))
        return ok, sum(mm + ov for mm, ov in counts), _score4(counts), dict(sum_mism=sum(mm for mm, _ in counts))

    return _select_survivors(hits, off, record, keep_best, VERIFY_STATS, SCORE_DTYPE)


def gapped_edits_host(transcripts, hits, offsets, reads1, reads2, max_indel):
    """The statement of a job's banded edit distance (csrc/verifygfmt.h restated in numpy).  Arguments as verify_hits_host; band k =
    max_indel (0 .. 15; 0 is the ungapped pass's diagonal alone).  For a job of len oriented bases a[] at pos on a transcript of tlen
    bases: cell (i, d), d = -k .. k, aligns read base i to x = pos + i + d; b(x) is the transcript's code for 0 <= x < tlen and OFF
    elsewhere; sub(i, x) = 0 iff a[i] <= 3 and b(x) == a[i], else 1.  D[-1][d] = 0 for every d; per row V[d] = min(D[i-1][d] +
    sub(i, pos + i + d), D[i-1][d+1] + 1) (the second term for d < k), then D[i][d] = min over d' <= d of V[d'] + (d - d'); edits =
    min over d of D[len-1][d], 0 for len == 0.  One row at a time, the band at once (and the jobs of one length side by side).
    -> (edits, ungapped): int64 arrays [records, 2], job 1's column 0 where a record has one job; ungapped = mism + over of
    verify_hits_host on the recorded diagonal.  ValueError naming the lowest record whose tid is not a transcript."""
    k = _max_indel(max_indel)
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    off = np.asarray(offsets).astype(np.int64)
    n_rec = int(off[-1]) if len(off) else 0
    bad = np.nonzero(hits["tid"][:n_rec] >= len(transcripts))[0]
    if len(bad):
        raise ValueError(f"record {int(bad[0])} names transcript >= {len(transcripts)}")
    OFF = 5
    d = np.arange(-k, k + 1, dtype=np.int64)
    ramp = np.arange(2 * k + 1, dtype=np.int64)
    tcodes = {}

    def same_length_jobs(jobs, n):
        """jobs: (read, fwd, tid, pos) of n bases each -> (edits, ungapped), the rows in step over all of them"""
        sub = np.empty((len(jobs), n, 2 * k + 1), np.int8)
        for j, (read, fwd, tid, pos) in enumerate(jobs):
            a = _oriented_codes(read, fwd)
            if tid not in tcodes:
                tcodes[tid] = _BASE_CODE[np.frombuffer(transcripts[tid], np.uint8)]
            t = tcodes[tid]
            x = pos + np.arange(n, dtype=np.int64)[:, None] + d[None, :]
            on = (x >= 0) & (x < len(t))
            b = np.full(x.shape, OFF, np.uint8)
            b[on] = t[x[on]]
            sub[j] = ~((a[:, None] <= 3) & (b == a[:, None]))
        D = np.zeros((len(jobs), 2 * k + 1), np.int64)
        for i in range(n):
            V = D + sub[:, i, :]
            if k:
                np.minimum(V[:, :-1], D[:, 1:] + 1, out=V[:, :-1])
            V -= ramp
            np.minimum.accumulate(V, axis=1, out=V)
            V += ramp
            D = V
        return D.min(axis=1), sub[:, :, k].astype(np.int64).sum(axis=1)

    by_len, where = {}, {}                             # the distinct jobs by length; (job) -> (length, index among them)
    slots = []
    for r in range(len(off) - 1):
        for i in range(off[r], off[r + 1]):
            for j, (rd, f, p) in enumerate(_record_jobs(hits[i], r, reads1, reads2)):
                key = (r, rd is not reads1[r], f, int(hits[i]["tid"]), p)
                if key not in where:
                    group = by_len.setdefault(len(rd), [])
                    where[key] = (len(rd), len(group))
                    group.append((rd, f, int(hits[i]["tid"]), p))
                slots.append((i, j, where[key]))
    done = {n: same_length_jobs(jobs, n) for n, jobs in by_len.items() if n}
    edits, ungapped = np.zeros((n_rec, 2), np.int64), np.zeros((n_rec, 2), np.int64)
    for i, j, (n, at) in slots:
        if n:
            edits[i, j], ungapped[i, j] = done[n][0][at], done[n][1][at]
    return edits, ungapped


def verify_hits_gapped_host(transcripts, hits, offsets, reads1, reads2, min_identity_permille, keep_best, max_indel, edits=None):
    """The statement of gapped hit verification (what sfgpu_hits_verify_gapped is judged by), on top of gapped_edits_host (whose
    result for the same batch and max_indel may be handed in as `edits`: it depends on neither permille nor keep_best).  A job passes
    iff 1000 (len - edits) >= permille len, a record iff all its jobs pass; keep_best keeps, of a read's passing records, those of
    least summed edits.  Score: {edits, ungapped, mate_edits, mate_ungapped}, saturating at 65 535, the mate fields 0 unless the status
    is 3.  Stats: VERIFYG_STATS -- `rescued` counts the survivors with a job that fails the ungapped rule 1000 (len - ungapped) >=
    permille len.  max_indel: 1 .. 15.  -> (hits, offsets uint32[R + 1], scores GSCORE_DTYPE, stats dict)"""
    k = _max_indel(max_indel)
    if k < 1:
        raise ValueError("max_indel lies outside 1 .. 15")
    permille = int(min_identity_permille)
    if not 0 <= permille <= 1000:
        raise ValueError("min_identity_permille lies outside 0 .. 1000")
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    off = np.asarray(offsets).astype(np.int64)
    ed, ung = gapped_edits_host(transcripts, hits, offsets, reads1, reads2, k) if edits is None else edits

    def record(r, i):
        lens = [len(rd) for rd, _, _ in _record_jobs(hits[i], r, reads1, reads2)]
        e, u = [int(v) for v in ed[i, :len(lens)]], [int(v) for v in ung[i, :len(lens)]]
        ok = all(1000 * (n - x) >= permille * n for n, x in zip(lens, e))
        rescued = any(1000 * (n - x) < permille * n for n, x in zip(lens, u))
        return ok, sum(e), _score4(zip(e, u)), dict(sum_edits=sum(e), rescued=int(rescued))

    return _select_survivors(hits, off, record, keep_best, VERIFYG_STATS, GSCORE_DTYPE)


def _device_reads(reads, dev):
    """(uint8 bases, int64 offsets) on the device, from such a pair or from a list of str / bytes"""
    if not isinstance(reads, tuple):
        from .mapper import pack_sequences
        reads = pack_sequences(reads)
    return reads[0].to(dev).contiguous(), reads[1].to(dev).contiguous()


def _device_batch(index, hits, offsets, reads1, reads2):
    """what verify_hits and align_hits hand the library: -> (device, hits, offsets, reads R, bases 1, offsets 1, bases 2 or None,
    offsets 2 or None, records n); ValueError where the reads and the hit offsets do not cover the same reads"""
    dev = index.device
    d_hits, d_off = _device_hits(hits, offsets, dev)
    R = int(d_off.numel()) - 1
    s1, o1 = _device_reads(reads1, dev)
    s2 = o2 = None
    if reads2 is not None:
        s2, o2 = _device_reads(reads2, dev)
    if int(o1.numel()) - 1 != R or (o2 is not None and int(o2.numel()) - 1 != R):
        raise ValueError("the reads and the hit offsets do not cover the same number of reads")
    return dev, d_hits, d_off, R, s1, o1, s2, o2, d_hits.numel() // 24


def _call_with_room(cap, make, call):
    """A library call whose output's size is known only afterwards.  make(cap) -> the tensor with room for cap; call(tensor, cap) ->
    (rc, need).  SFGPU_ERR_RANGE with a need above cap: repeated once, with exactly that room; then _lib.check.  -> (tensor, need)"""
    for attempt in range(2):
        out = make(cap)
        rc, need = call(out, cap)
        if rc != _lib.ERR_RANGE or attempt or need <= cap:
            break
        cap = int(need)
    _lib.check(rc)
    return out, need


def verify_hits(index, hits, offsets, reads1, reads2=None, *, min_identity=0.9, keep_best=False, max_indel=0):
    """Verify the mapper's hit records against the transcripts' bases on the device (sfgpu_hits_verify; the rules are
    verify_hits_host's).  index: the mapper.QuasiIndex the records come from; hits / offsets: device tensors as QuasiIndex.map_reads
    returns them; reads1 / reads2: the batch's reads, packed (bases, offsets) pairs or lists, as map_reads takes them.  A job passes
    with at least min_identity of its bases equal to the transcript's on the recorded diagonal (the permille is
    int(round(min_identity * 1000)); outside 0 .. 1000: ValueError); keep_best keeps only a read's records of least mism + over.
    max_indel = 1 .. 15 scores with gaps instead (sfgpu_hits_verify_gapped; the rules are verify_hits_gapped_host's): a job's cost is
    its banded edit distance, within max_indel diagonals of the recorded one and with a free start diagonal, so a read with an indel
    keeps its true record; the scores are then GSCORE_DTYPE records and the stats VERIFYG_STATS.  The records are returned as they
    came: pos still names the recorded diagonal.  Anything else than 0 .. 15: ValueError.
    -> (hits, offsets, scores: uint8 device tensor of SCORE_DTYPE records, stats dict)"""
    permille = _permille(min_identity)
    k = _max_indel(max_indel)
    dev, d_hits, d_off, R, s1, o1, s2, o2, n = _device_batch(index, hits, offsets, reads1, reads2)
    out_hits = torch.empty(max(n, 1) * 24, dtype=torch.uint8, device=dev)
    out_off = torch.empty(R + 1, dtype=torch.int32, device=dev)
    scores = torch.empty(max(n, 1) * 8, dtype=torch.uint8, device=dev)
    o = _lib.VerifyGOpts(permille, int(bool(keep_best)), k) if k else _lib.VerifyOpts(permille, int(bool(keep_best)))
    st = _lib.VerifyGStats() if k else _lib.VerifyStats()
    entry = _lib.lib().sfgpu_hits_verify_gapped if k else _lib.lib().sfgpu_hits_verify
    n_out = C.c_uint64(0)
    with torch.cuda.device(dev):
        torch.cuda.current_stream().synchronize()
        _lib.check(entry(index._h, _lib.ptr(s1), _lib.ptr(o1), _lib.ptr(s2), _lib.ptr(o2), R, _lib.ptr(d_hits), _lib.ptr(d_off),
                         C.byref(o), _lib.ptr(out_hits), _lib.ptr(out_off), _lib.ptr(scores), C.byref(n_out), C.byref(st), _lib.current_stream_ptr()))
    return out_hits[: n_out.value * 24], out_off, scores[: n_out.value * 8], st.as_dict()


RESCUE_STATS = ("reads_eligible", "records_orphan", "jobs_with_candidates", "candidates", "reads_rescued", "records_rescued", "records_dropped", "sum_mism")
MAX_RESCUE_WINDOW = 1 << 20


def _rescue_window(window):
    w = int(window)
    if w != window or not 1 <= w <= MAX_RESCUE_WINDOW:
        raise ValueError(f"window = {window!r} is no integer in 1 .. {MAX_RESCUE_WINDOW}")
    return w


def rescue_mates_host(transcripts, hits, offsets, reads1, reads2, min_identity_permille, window):
    """The statement of mate rescue (csrc/rescuefmt.h restated in numpy; what sfgpu_hits_rescue_mates is judged by).  Arguments as
    verify_hits_host, of a paired batch (reads2 is None: ValueError); window = W, 1 .. 2^20.  A read is eligible iff it has a record
    and every record has mate_status 1 or 2; every other read keeps its records.  A job is one orphan record of an eligible read: the
    anchor (mate 1 for status 1, mate 2 for status 2; la bases) sits at p = pos on strand f = fwd, the missing mate (the other one, lb
    bases) is oriented on strand 1 - f.  Candidates are the x with 0 <= x <= tlen - lb and, f == 1: x >= p and x + lb <= p + W; f == 0:
    x + lb <= p + la and x >= p + la - W; lb == 0, lb > tlen, lb > 65 535 and la > 65 535 give none.  mism(x) counts the columns where
    either code is 4 or the codes differ; a candidate passes iff 1000 (lb - mism) >= permille lb; the placement is the passing
    candidate of least mism, the lowest x on a tie.  A placed job yields the pair record -- status 1: (tid, p, x, frag, len1, len2, f,
    1 - f, 3, 0); status 2: (tid, x, p, frag, len1, len2, 1 - f, f, 3, 0); frag = max(ends) - min(starts).  A read with a placed job
    keeps its placed records only, ordered by (tid, fwd) and by input order on equal keys; a read without keeps its orphans.
    -> (hits, offsets uint32[R + 1], mism uint16 per output record: the placed mate's, saturated, 0 for records passed through,
    stats dict of RESCUE_STATS); ValueError naming the lowest record whose tid is not a transcript."""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    off = np.asarray(offsets).astype(np.int64)
    permille, W = int(min_identity_permille), _rescue_window(window)
    if not 0 <= permille <= 1000:
        raise ValueError("min_identity_permille lies outside 0 .. 1000")
    if reads2 is None:
        raise ValueError("a single-end batch has no mates to rescue")
    n_rec = int(off[-1]) if len(off) else 0
    bad = np.nonzero(hits["tid"][:n_rec] >= len(transcripts))[0]
    if len(bad):
        raise ValueError(f"record {int(bad[0])} names transcript >= {len(transcripts)}")
    stats = dict.fromkeys(RESCUE_STATS, 0)
    tcodes = {}
    out, mism_out, out_off = [], [], [0]
    for r in range(len(off) - 1):
        recs = [hits[i] for i in range(off[r], off[r + 1])]
        placed = []
        if recs and all(int(h["mate_status"]) in (1, 2) for h in recs):
            stats["reads_eligible"] += 1
            stats["records_orphan"] += len(recs)
            len1, len2 = len(reads1[r]), len(reads2[r])
            for n, h in enumerate(recs):
                st, tid, p, f = int(h["mate_status"]), int(h["tid"]), int(h["pos"]), int(h["fwd"] != 0)
                la, lb, mate = (len1, len2, reads2[r]) if st == 1 else (len2, len1, reads1[r])
                if tid not in tcodes:
                    tcodes[tid] = _BASE_CODE[np.frombuffer(transcripts[tid], np.uint8)]
                t = tcodes[tid]
                if lb == 0 or lb > len(t) or lb > 65535 or la > 65535:
                    continue
                lo, hi = (p, p + W - lb) if f else (p + la - W, p + la - lb)
                lo, hi = max(lo, 0), min(hi, len(t) - lb)
                if hi < lo:
                    continue
                stats["jobs_with_candidates"] += 1
                stats["candidates"] += hi - lo + 1
                q = _oriented_codes(mate, not f)
                win = np.lib.stride_tricks.sliding_window_view(t[lo:hi + lb], lb)
                mm = ((win != q) | (win > 3) | (q > 3)).sum(axis=1)
                ok = np.nonzero(1000 * (lb - mm) >= permille * lb)[0]
                if not len(ok):
                    continue
                at = int(ok[np.argmin(mm[ok])])                       # (argmin: the first of the least)
                x, m = lo + at, int(mm[at])
                frag = (max(p + la, x + lb) - min(p, x)) & 0xFFFFFFFF
                rec = (tid, p, x, frag, len1, len2, f, 1 - f, 3, 0) if st == 1 else (tid, x, p, frag, len1, len2, 1 - f, f, 3, 0)
                placed.append(((tid, rec[6], n), rec, m))
        if placed:
            stats["reads_rescued"] += 1
            stats["records_rescued"] += len(placed)
            stats["records_dropped"] += len(recs) - len(placed)
            for _, rec, m in sorted(placed, key=lambda v: v[0]):
                out.append(rec)
                mism_out.append(min(m, 65535))
                stats["sum_mism"] += m
        else:
            out.extend(h.tolist() for h in recs)
            mism_out.extend([0] * len(recs))
        out_off.append(len(out))
    return np.array(out, dtype=HIT_DTYPE), np.array(out_off, np.uint32), np.array(mism_out, np.uint16), stats


def rescue_mates(index, hits, offsets, reads1, reads2, *, min_identity=0.9, window=1000):
    """Rescue the missing mates of orphan-only reads on the device (sfgpu_hits_rescue_mates; the rules are rescue_mates_host's).
    index, hits / offsets, reads1 / reads2 as verify_hits takes them, of a paired batch.  Every orphan record of a read that has
    nothing but orphans has its transcript searched for the other mate -- ungapped, on the opposite strand, inside the window an
    inward-facing fragment of at most `window` bases (1 .. 2^20, else ValueError) allows; a placement needs at least min_identity of
    the mate's bases equal to the transcript's (the permille is int(round(min_identity * 1000)); outside 0 .. 1000: ValueError).  A
    read with a placement keeps its placed records, as PAIRED_END_PAIRED records in the mapper's form and order; every other read
    keeps what it had.
    -> (hits, offsets, mism: uint8 device tensor of '<u2' values, one per output record, stats dict)"""
    permille = _permille(min_identity)
    W = _rescue_window(window)
    if reads2 is None:
        raise ValueError("a single-end batch has no mates to rescue")
    dev, d_hits, d_off, R, s1, o1, s2, o2, n = _device_batch(index, hits, offsets, reads1, reads2)
    out_off = torch.empty(R + 1, dtype=torch.int32, device=dev)
    mism = torch.empty(max(n, 1) * 2, dtype=torch.uint8, device=dev)
    o, st, n_out = _lib.RescueOpts(permille, W), _lib.RescueStats(), C.c_uint64(0)

    def call(out_hits, cap):                             # (never more records than came in: the room is known beforehand)
        rc = _lib.lib().sfgpu_hits_rescue_mates(index._h, _lib.ptr(s1), _lib.ptr(o1), _lib.ptr(s2), _lib.ptr(o2), R, _lib.ptr(d_hits), _lib.ptr(d_off),
                                                C.byref(o), _lib.ptr(out_hits), _lib.ptr(out_off), _lib.ptr(mism), C.byref(n_out), C.byref(st), _lib.current_stream_ptr())
        return rc, n_out.value
    with torch.cuda.device(dev):
        torch.cuda.current_stream().synchronize()
        out_hits, total = _call_with_room(max(n, 1), lambda cap: torch.empty(cap * 24, dtype=torch.uint8, device=dev), call)
    return out_hits[: total * 24], out_off, mism[: total * 2], st.as_dict()


ALIGNG_STATS = ("jobs", "jobs_traced", "unalignable", "sum_nm", "words", "scratch_bytes")
CIGAR_M, CIGAR_I, CIGAR_D, CIGAR_S = 0, 1, 2, 4                                       # BAM's operation codes
_DIAG, _INS, _DEL = 1, 2, 4


def _align_job_host(a, t, pos, k):
    """One job by the rule of csrc/aligngfmt.h: a = the oriented base codes, t = the transcript's codes -> (x0, ops, nm, clipped,
    trimmed D columns, edits, ungapped count).  The whole matrix D[i][d] (gapped_edits_host's rows, kept), then CANDIDATES, END, WALK, TRIM, RESULT."""
    n, tl = len(a), len(t)
    if n == 0:
        return 0, [], 0, 0, 0, 0, 0
    d = np.arange(-k, k + 1, dtype=np.int64)
    ramp = np.arange(2 * k + 1, dtype=np.int64)
    x = pos + np.arange(n, dtype=np.int64)[:, None] + d[None, :]
    on = (x >= 0) & (x < tl)
    b = np.full(x.shape, 5, np.uint8)
    b[on] = t[x[on]]
    sub = (~((a[:, None] <= 3) & (b == a[:, None]))).astype(np.int64)
    D = np.zeros((n + 1, 2 * k + 1), np.int64)                                        # row i is D[i + 1]
    for i in range(n):
        V = D[i] + sub[i]
        np.minimum(V[:-1], D[i, 1:] + 1, out=V[:-1])
        V -= ramp
        np.minimum.accumulate(V, out=V)
        V += ramp
        D[i + 1] = V
    ungapped = int(sub[:, k].sum())
    D, sub = D.tolist(), sub.tolist()
    edits = min(D[n])
    l = next(c for m in range(k + 1) for c in (k - m, k + m) if D[n][c] == edits)      # END: least |d|, the negative one on a tie
    cols, i, prev = [], n - 1, 0
    while i >= 0:                                                                      # WALK
        here = D[i + 1][l]
        diag = D[i][l] + sub[i][l] == here
        ins = l < 2 * k and D[i][l + 1] + 1 == here
        dele = l > 0 and D[i + 1][l - 1] + 1 == here
        op = _DEL if prev == _DEL and dele else _INS if prev == _INS and ins else _DIAG if diag else _INS if ins else _DEL
        xx = pos + i + l - k
        if op == _DIAG:
            cols.append((CIGAR_M, xx, sub[i][l])); i -= 1
        elif op == _INS:
            cols.append((CIGAR_I, xx, 1)); i -= 1; l += 1
        else:
            cols.append((CIGAR_D, xx, 1)); l -= 1
        prev = op
    cols.reverse()
    remains = [c[0] == CIGAR_M and 0 <= c[1] < tl for c in cols]                      # TRIM
    if not any(remains):
        return 0, [], 0, n, sum(c[0] == CIGAR_D for c in cols), edits, ungapped
    lo, hi = remains.index(True), len(cols) - remains[::-1].index(True)
    dropped = cols[:lo] + cols[hi:]
    clip_l, clip_r = sum(c[0] != CIGAR_D for c in cols[:lo]), sum(c[0] != CIGAR_D for c in cols[hi:])
    ops = [clip_l << 4 | CIGAR_S] if clip_l else []
    last = None
    for kind, _, _ in cols[lo:hi]:
        if kind == last:
            ops[-1] += 1 << 4
        else:
            ops.append(1 << 4 | kind)
        last = kind
    if clip_r:
        ops.append(clip_r << 4 | CIGAR_S)
    return cols[lo][1], ops, sum(c[2] for c in cols[lo:hi]), clip_l + clip_r, sum(c[0] == CIGAR_D for c in dropped), edits, ungapped


def align_hits_host(transcripts, hits, offsets, reads1, reads2, max_indel):
    """The statement of gapped alignment (csrc/aligngfmt.h restated; what sfgpu_hits_align_gapped is judged by), extending
    gapped_edits_host: the same cells, then for each job the walk back through the band -- from the cell of the last row that holds
    the edits with least |d| (the negative d on a tie); a gap continued while it is a candidate, else the first candidate of DIAG,
    INS, DEL -- trimmed at either end to the first base aligned on the transcript (dropped bases are soft clip, dropped D columns
    vanish; nothing left: unalignable, no operations).  Arguments as verify_hits_host; max_indel 1 .. 15.  Two slots per record: slot
    2 h + j is job j of record h, a missing second job an empty slot.
    -> (pos int32[2 n], nm uint32[2 n], op_off uint64[2 n + 1], ops uint32[] of len << 4 | op with M 0, I 1, D 2, S 4,
        stats dict (ALIGNG_STATS; scratch_bytes as of one slice), detail int64[2 n, 3]: clipped, trimmed D columns, edits);
    nm + clipped + trimmed D == edits in every slot.  ValueError naming the lowest record whose tid is not a transcript."""
    k = _max_indel(max_indel)
    if k < 1:
        raise ValueError("max_indel lies outside 1 .. 15")
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    off = np.asarray(offsets).astype(np.int64)
    n_rec = int(off[-1]) if len(off) else 0
    bad = np.nonzero(hits["tid"][:n_rec] >= len(transcripts))[0]
    if len(bad):
        raise ValueError(f"record {int(bad[0])} names transcript >= {len(transcripts)}")
    width = 16 if k <= 7 else 32
    tcodes, done = {}, {}
    pos, nm = np.zeros(2 * n_rec, np.int32), np.zeros(2 * n_rec, np.uint32)
    op_off, ops = np.zeros(2 * n_rec + 1, np.uint64), []
    detail = np.zeros((2 * n_rec, 3), np.int64)
    stats = dict.fromkeys(ALIGNG_STATS, 0)
    for r in range(len(off) - 1):
        for i in range(off[r], off[r + 1]):
            tid = int(hits[i]["tid"])
            if tid not in tcodes:
                tcodes[tid] = _BASE_CODE[np.frombuffer(transcripts[tid], np.uint8)]
            for j, (rd, fwd, p) in enumerate(_record_jobs(hits[i], r, reads1, reads2)):
                key = (r, rd is not reads1[r], fwd, tid, p)
                if key not in done:
                    done[key] = _align_job_host(_oriented_codes(rd, fwd), tcodes[tid], p, k)
                x0, job_ops, job_nm, clipped, trimmed, edits, ungapped = done[key]
                s = 2 * i + j
                pos[s], nm[s], detail[s] = x0, job_nm, (clipped, trimmed, edits)
                ops.extend(job_ops)
                op_off[s + 1] = len(job_ops)
                stats["jobs"] += 1
                stats["jobs_traced"] += int(ungapped > 0)
                stats["unalignable"] += int(not job_ops)
                stats["sum_nm"] += job_nm
                if ungapped > 0:
                    stats["scratch_bytes"] += 8 * width * ((len(rd) + 15) // 16)
    op_off = np.cumsum(op_off, dtype=np.uint64)
    stats["words"] = len(ops)
    return pos, nm, op_off, np.array(ops, np.uint32), stats, detail


def align_hits(index, hits, offsets, reads1, reads2=None, *, max_indel, scratch_cap_bytes=0):
    """The gapped alignment of hit records on the device (sfgpu_hits_align_gapped; the rule is align_hits_host's): for the records
    that verify_hits(max_indel=) kept, the path through the same band as a position and CIGAR words per job.  Arguments as
    verify_hits; max_indel 1 .. 15 (anything else: ValueError).  scratch_cap_bytes bounds the device scratch of one slice of the batch
    (0: 256 MiB); it never changes a result.  The operations' room is sized at two words a slot and the call repeated once with the
    count the library reports where they do not fit.
    -> (pos int32[2 n], nm int32[2 n] (the bits of uint32), op_off int64[2 n + 1], ops int32[] (the bits of uint32), stats dict):
    device tensors, two slots per record (slot 2 h + j is job j of record h)."""
    k = _max_indel(max_indel)
    if k < 1:
        raise ValueError("max_indel lies outside 1 .. 15")
    dev, d_hits, d_off, R, s1, o1, s2, o2, n = _device_batch(index, hits, offsets, reads1, reads2)
    pos = torch.zeros(2 * n, dtype=torch.int32, device=dev)
    nm = torch.zeros(2 * n, dtype=torch.int32, device=dev)
    op_off = torch.zeros(2 * n + 1, dtype=torch.int64, device=dev)
    o = _lib.AlignGOpts(k, 0, int(scratch_cap_bytes))
    st = _lib.AlignGStats()
    need = C.c_uint64(0)

    def call(ops, cap):
        rc = _lib.lib().sfgpu_hits_align_gapped(index._h, _lib.ptr(s1), _lib.ptr(o1), _lib.ptr(s2), _lib.ptr(o2), R, _lib.ptr(d_hits), _lib.ptr(d_off),
                                                C.byref(o), _lib.ptr(pos), _lib.ptr(nm), _lib.ptr(op_off), _lib.ptr(ops), cap, C.byref(need), C.byref(st),
                                                _lib.current_stream_ptr())
        return rc, need.value
    with torch.cuda.device(dev):
        torch.cuda.current_stream().synchronize()
        ops, n_ops = _call_with_room(max(4 * n, 1), lambda cap: torch.empty(cap, dtype=torch.int32, device=dev), call)
    return pos, nm, op_off, ops[:n_ops], st.as_dict()


MDTAG_STATS = ("slots", "sum_nm", "md_bytes", "max_md_bytes", "slots_plain")
_MATCH_OPS, _DEL_OPS = (0, 7, 8), (2, 3)                                              # M = X; D N


def _md_ref_char(t, x):
    """the reference character of csrc/mdfmt.h: the transcript's byte upper-cased, N where that is no letter or off the transcript"""
    if x < 0 or x >= len(t):
        return 78
    b = t[x] - 32 if 97 <= t[x] <= 122 else t[x]
    return b if 65 <= b <= 90 else 78


def _md_slot_host(words, x, a, t, tcode):
    """One slot by the rule of csrc/mdfmt.h: words = the line's CIGAR (len << 4 | op), x = POS - 1, a = the mate's oriented codes,
    t / tcode = the transcript's bytes and codes -> (nm, the MD's bytes)"""
    q, run, nm, md = 0, 0, 0, bytearray()
    for w in words:
        n, op = int(w) >> 4, int(w) & 15
        if op == CIGAR_S:
            q += n
        elif op == CIGAR_I:
            q += n; nm += n
        elif op in _DEL_OPS:
            md += b"%d^" % run
            md += bytes(_md_ref_char(t, x + j) for j in range(n))
            run = 0; nm += n; x += n
        elif op in _MATCH_OPS:
            for _ in range(n):
                if x < 0 or x >= len(t) or q >= len(a) or a[q] > 3 or tcode[x] > 3 or a[q] != tcode[x]:
                    md += b"%d" % run
                    md.append(_md_ref_char(t, x))
                    run = 0; nm += 1
                else:
                    run += 1
                q += 1; x += 1
    md += b"%d" % run
    return nm, bytes(md)


def md_tags_host(transcripts, hits, offsets, reads1, reads2, alignments=None):
    """The statement of the NM and MD tags of a mappings file's lines (csrc/mdfmt.h restated; what sfgpu_hits_md_tags is judged by),
    in plain loops.  Arguments as verify_hits_host; alignments: what align_hits / align_hits_host returned for the same records
    (pos, nm, op_off, ops, ...), or None.  Two slots per record: slot 2 h + which is line `which` of record h, its mate, strand and
    bases those of _record_jobs.  The line's CIGAR is the one the writer writes: the slot's words at POS - 1 = pos[slot] with an
    alignment, else <clip>S<match>M from the record's pos and read_len (mate_pos and mate_len on the second line); a line the writer
    refuses (no base on the transcript, a slot without an operation) has no operation: nm 0, MD "0".  It is walked over the oriented
    mate: S skips read bases; an M / = / X column off the transcript, past the mate's bases, with a base that is not A C G T, or with
    differing bases is <run><reference character> and nm + 1, else the run grows; I n is nm + n; D n / N n is <run>^<n reference
    characters> and nm + n; <run> ends the MD.  A record's missing second slot has nm 0 and an empty MD.
    -> (nm uint32[2 n], md_off uint64[2 n + 1], md uint8[], stats dict (MDTAG_STATS)).  ValueError naming the lowest record whose
    tid is not a transcript."""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    off = np.asarray(offsets).astype(np.int64)
    n_rec = int(off[-1]) if len(off) else 0
    bad = np.nonzero(hits["tid"][:n_rec] >= len(transcripts))[0]
    if len(bad):
        raise ValueError(f"record {int(bad[0])} names transcript >= {len(transcripts)}")
    aln = None
    if alignments is not None:
        host = lambda v, dt: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)).view(dt).reshape(-1)
        aln = host(alignments[0], np.int32), host(alignments[2], np.uint64), host(alignments[3], np.uint32)
        if len(aln[0]) != 2 * n_rec or len(aln[1]) != 2 * n_rec + 1:
            raise ValueError(f"an alignment of {len(aln[0])} slots for {n_rec} records (two slots a record)")
    nm, md_off, md = np.zeros(2 * n_rec, np.uint32), np.zeros(2 * n_rec + 1, np.uint64), []
    stats = dict.fromkeys(MDTAG_STATS, 0)
    tcodes = {}
    for r in range(len(off) - 1):
        for i in range(off[r], off[r + 1]):
            h = hits[i]
            tid = int(h["tid"])
            if tid not in tcodes:
                tcodes[tid] = _BASE_CODE[np.frombuffer(transcripts[tid], np.uint8)].tolist()
            for j, (rd, fwd, _) in enumerate(_record_jobs(h, r, reads1, reads2)):
                s = 2 * i + j
                if aln is not None:
                    words, x = aln[2][int(aln[1][s]):int(aln[1][s + 1])].tolist(), int(aln[0][s])
                else:
                    pos, length = (int(h["mate_pos"]), int(h["mate_len"])) if j else (int(h["pos"]), int(h["read_len"]))
                    if pos >= 0:
                        words, x = [length << 4], pos
                    elif -pos < length:
                        words, x = [-pos << 4 | CIGAR_S, (length + pos) << 4], 0
                    else:
                        words, x = [], 0
                got, text = _md_slot_host(words, x, _oriented_codes(rd, fwd).tolist(), transcripts[tid], tcodes[tid])
                nm[s], md_off[s + 1] = got, len(text)
                md.append(text)
                stats["slots"] += 1
                stats["sum_nm"] += got
                stats["md_bytes"] += len(text)
                stats["max_md_bytes"] = max(stats["max_md_bytes"], len(text))
                stats["slots_plain"] += int(len(words) == 1 and words[0] & 15 == CIGAR_M and got == 0)
    return nm, np.cumsum(md_off, dtype=np.uint64), np.frombuffer(b"".join(md), np.uint8), stats


def md_tags(index, hits, offsets, reads1, reads2=None, alignments=None):
    """The NM and MD tags of hit records on the device (sfgpu_hits_md_tags; the rule is md_tags_host's).  Arguments as verify_hits;
    alignments: what align_hits returned for the same records (pos, nm, op_off, ops, ...) or None for the ungapped lines.  The MD's
    room is sized at four bytes a slot and the call repeated once with the count the library reports where they do not fit.
    -> (nm int32[2 n] (the bits of uint32), md_off int64[2 n + 1], md uint8[], stats dict (MDTAG_STATS)): device tensors, two slots
    per record (slot 2 h + which is line `which` of record h).  NH is no output: it is the read's record count, offsets[r + 1] -
    offsets[r]."""
    dev, d_hits, d_off, R, s1, o1, s2, o2, n = _device_batch(index, hits, offsets, reads1, reads2)
    a_pos = a_off = a_ops = None
    if alignments is not None:
        signed = {4: np.int32, 8: np.int64}
        a_pos, a_off, a_ops = ((v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v).view(signed[v.dtype.itemsize]).copy())).to(dev).contiguous()
                               for v in (alignments[0], alignments[2], alignments[3]))
        if int(a_pos.numel()) != 2 * n or int(a_off.numel()) != 2 * n + 1:
            raise ValueError(f"an alignment of {int(a_pos.numel())} slots for {n} records (two slots a record)")
        if int(a_ops.numel()) == 0:
            a_ops = torch.zeros(1, dtype=torch.int32, device=dev)
    nm = torch.zeros(2 * n, dtype=torch.int32, device=dev)
    md_off = torch.zeros(2 * n + 1, dtype=torch.int64, device=dev)
    st = _lib.MdTagStats()
    need = C.c_uint64(0)

    def call(md, cap):
        rc = _lib.lib().sfgpu_hits_md_tags(index._h, _lib.ptr(s1), _lib.ptr(o1), _lib.ptr(s2), _lib.ptr(o2), R, _lib.ptr(d_hits), _lib.ptr(d_off),
                                           _lib.ptr(a_pos), _lib.ptr(a_off), _lib.ptr(a_ops), _lib.ptr(nm), _lib.ptr(md_off), _lib.ptr(md), cap,
                                           C.byref(need), C.byref(st), _lib.current_stream_ptr())
        return rc, need.value
    with torch.cuda.device(dev):
        torch.cuda.current_stream().synchronize()
        md, n_md = _call_with_room(max(8 * n, 1), lambda cap: torch.empty(cap, dtype=torch.uint8, device=dev), call)
    return nm, md_off, md[:n_md], st.as_dict()


POSTERIOR_STATS = ("reads", "reads_mapped", "reads_multi", "records", "reads_flat", "records_zero", "max_records")
POST_TINY, POST_HUGE, POST_FLUSH = 2.0 ** -960, 2.0 ** 960, 2.0 ** -56
_POST_XOR = [np.arange(64) ^ k for k in (32, 16, 8, 4, 2, 1)]


def post_sum_host(x):
    """csrc/postfmt.h's SUM of float64 values: 64 accumulators a_j = x_j + x_{j+64} + ..., serially and ascending (0 where there
    is no x_j), then a_j <- a_j + a_{j xor k} for k = 32, 16, 8, 4, 2, 1 and every j at once; a_0"""
    a = np.zeros(64, np.float64)
    for i in range(0, len(x), 64):
        seg = x[i:i + 64]
        a[:len(seg)] = a[:len(seg)] + seg
    for perm in _POST_XOR:
        a = a + a[perm]
    return float(a[0])


def posterior_record(p):
    """csrc/gfmt.h's six-digit record of a value 0 or 2^-56 .. 1, read off Python's own '%.5e': the digits without their trailing
    zeros in bits 0 .. 19, the decimal exponent + 512 in bits 20 .. 29; bit 31 alone for 0"""
    if p == 0:
        return 1 << 31
    mant, exp = ("%.5e" % p).split("e")
    return int(mant.replace(".", "").rstrip("0")) | (int(exp) + 512) << 20


def posterior_token(rec):
    """the '%g' token of such a record, placed from its digits alone (what the writers' formatter does with it)"""
    rec = int(rec) & 0xFFFFFFFF
    if rec >> 31:
        return "0"
    d, x = str(rec & 0xFFFFF), ((rec >> 20) & 0x3FF) - 512
    if -4 <= x < 6:
        if x < 0:
            return "0." + "0" * (-x - 1) + d
        return d + "0" * (x + 1 - len(d)) if len(d) <= x + 1 else d[:x + 1] + "." + d[x + 1:]
    return d[0] + ("." + d[1:] if len(d) > 1 else "") + "e%+03d" % x


def posteriors_host(hits, offsets, weights):
    """The statement of the posterior pass (csrc/postfmt.h restated; what sfgpu_hits_posteriors is judged by).  hits: HIT_DTYPE
    records in CSR form over the reads (offsets[R + 1]); weights: float64 per transcript.  For a read's n records x_h =
    weights[tid_h], a weight below 2^-960 reading as 0 and every record a term of its own; S = post_sum_host(x); p_h = x_h / S where
    S > 0, else 1 / n; a p_h below 2^-56 is written as 0.  The token is '%g' % p_h, rec its six-digit record (posterior_record) and
    f32 the float32 nearest to float(token): what a BAM reader gets from the token.
    -> (p float64[n], rec uint32[n], f32 float32[n], stats dict of POSTERIOR_STATS).  ValueError naming the lowest transcript whose
    weight is negative, NaN, infinite or above 2^960, else the lowest record whose tid is not a transcript."""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    off = np.asarray(offsets).astype(np.int64)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    n_rec = int(off[-1]) if len(off) else 0
    with np.errstate(invalid="ignore"):
        bad = np.nonzero(~(w >= 0) | (w > POST_HUGE))[0]
    if len(bad):
        raise ValueError(f"the weight of transcript {int(bad[0])} is negative, not finite or above 2^960")
    bad = np.nonzero(hits["tid"][:n_rec] >= len(w))[0]
    if len(bad):
        raise ValueError(f"record {int(bad[0])} names transcript >= {len(w)}")
    x_all = np.where(w < POST_TINY, 0.0, w)[hits["tid"][:n_rec].astype(np.int64)] if n_rec else np.zeros(0)
    p = np.zeros(n_rec, np.float64)
    sizes = np.diff(off) if len(off) else np.zeros(0, np.int64)
    stats = dict(reads=len(sizes), reads_mapped=int((sizes >= 1).sum()), reads_multi=int((sizes >= 2).sum()), records=n_rec, reads_flat=0,
                 records_zero=0, max_records=int(sizes.max()) if len(sizes) else 0)
    for r in np.nonzero(sizes)[0]:
        x = x_all[off[r]:off[r + 1]]
        s = post_sum_host(x)
        stats["reads_flat"] += int(not s > 0)
        p[off[r]:off[r + 1]] = x / s if s > 0 else 1.0 / len(x)
    p[p < POST_FLUSH] = 0.0
    stats["records_zero"] = int((p == 0).sum())
    rec = np.array([posterior_record(v) for v in p.tolist()], np.uint32)
    f32 = np.array([float("%g" % v) for v in p.tolist()], np.float64).astype(np.float32)
    return p, rec, f32, stats


def posteriors(hits, offsets, weights, device="cuda"):
    """The posterior probability of every hit record under a weight per transcript, on the device (sfgpu_hits_posteriors; the rule is
    posteriors_host's).  hits / offsets: device tensors as QuasiIndex.map_reads returns them (or host arrays); weights: a float64
    tensor or array, one per transcript, on the device of `hits` where that is a tensor.
    -> (p float64[n], rec int32[n] (the bits of uint32: the six-digit record of '%g' % p), f32 float32[n], stats dict
    (POSTERIOR_STATS)): device tensors, one entry per record."""
    dev = hits.device if isinstance(hits, torch.Tensor) and hits.is_cuda else torch.device(device)
    d_hits, d_off = _device_hits(hits, offsets, dev)
    w = (weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(weights, np.float64).copy())).to(dev, torch.float64).contiguous()
    R, n = int(d_off.numel()) - 1, d_hits.numel() // 24
    if R < 0:
        raise ValueError("hit offsets hold at least one entry")
    p = torch.zeros(n, dtype=torch.float64, device=dev)
    rec = torch.zeros(n, dtype=torch.int32, device=dev)
    f32 = torch.zeros(n, dtype=torch.float32, device=dev)
    st = _lib.PosteriorStats()
    with torch.cuda.device(dev):
        torch.cuda.current_stream().synchronize()
        _lib.check(_lib.lib().sfgpu_hits_posteriors(_lib.ptr(d_hits), _lib.ptr(d_off), R, _lib.ptr(w), int(w.numel()), _lib.ptr(p), _lib.ptr(rec), _lib.ptr(f32),
                                                    C.byref(st), _lib.current_stream_ptr()))
    return p, rec, f32, st.as_dict()


LIBDET_KINDS = ("ISF", "ISR", "OSF", "OSR", "MSF", "MSR", "LF", "LR", "RF", "RR", "SF", "SR", "other")
LIBDET_STATS = ("reads", "reads_mapped", "reads_over_occs", "reads_mixed", "reads_compatible", "votes", "records_kind", "reads_kind", "votes_kind")
LIBDET_PERMILLE = (501, 1000)
_FORMAT_NAMES = {v: k for k, v in LIBRARY_FORMATS.items()}


def _libdet_stats(stats=None):
    """a fresh set of the counters, or a copy of `stats` to add to"""
    if stats is None:
        return {k: [0] * len(LIBDET_KINDS) if k.endswith("_kind") else 0 for k in LIBDET_STATS}
    return {k: [int(v) for v in stats[k]] if k.endswith("_kind") else int(stats[k]) for k in LIBDET_STATS}


def _libdet_permille(min_fraction):
    p = int(round(float(min_fraction) * 1000))
    if not LIBDET_PERMILLE[0] <= p <= LIBDET_PERMILLE[1]:
        raise ValueError(f"min_fraction = {min_fraction!r} lies outside 0.501 .. 1")
    return p


def _format_triple(lib_format):
    return LIBRARY_FORMATS[lib_format.upper()] if isinstance(lib_format, str) else tuple(int(v) for v in lib_format)


def record_kinds_host(hits, allow_dovetail=False):
    """csrc/libdetfmt.h's KIND of every record, restated in numpy: an index into LIBDET_KINDS each.  Status 3: the mates' starts s1, s2
    are pos (forward) or pos + len (reverse), the sum taken in uint32 and read as int32; mates on different strands are *SF where mate 1
    is the forward one, inward iff s1 <= s2 + stretch (*SR: s2 <= s1 + stretch), stretch being the other mate's length with
    allow_dovetail, else 0; mates on one strand are MSF / MSR.  Status 1 / 2 / 0: LF LR / RF RR / SF SR.  Any other status: other."""
    h = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    st, f1, f2 = h["mate_status"], h["fwd"] != 0, h["mate_fwd"] != 0

    def start(pos, length, fwd):
        s = (pos.astype(np.int64) + np.where(fwd, 0, length.astype(np.int64))) & 0xFFFFFFFF
        return np.where(s >= 1 << 31, s - (1 << 32), s)
    s1, s2 = start(h["pos"], h["read_len"], f1), start(h["mate_pos"], h["mate_len"], f2)
    stretch1 = h["mate_len"].astype(np.int64) if allow_dovetail else 0
    stretch2 = h["read_len"].astype(np.int64) if allow_dovetail else 0
    pair = np.where(f1 == f2, np.where(f1, 4, 5), np.where(f1, np.where(s1 <= s2 + stretch1, 0, 2), np.where(s2 <= s1 + stretch2, 1, 3)))
    rev = (~f1).astype(np.int64)
    return np.select([st == 3, st == 1, st == 2, st == 0], [pair, 6 + rev, 8 + rev, 10 + rev], 12).astype(np.uint8)


def kind_compatible(lib_format, kind):
    """does the library format accept a record of this kind (a LIBDET_KINDS name or index)?  What compatibleHit says of it: a pair
    must show the format's orientation and, unless that is unstranded, its strandedness; a single-end read and an orphan must lie on
    the strand the format puts that mate on (a right orphan of an inward or outward library on the opposite one)."""
    _, eo, es = _format_triple(lib_format)
    k = LIBDET_KINDS.index(kind) if isinstance(kind, str) else int(kind)
    if k <= 5:
        oo = (TOWARD, AWAY, SAME)[k // 2]
        os_ = (S, A)[k & 1] if oo == SAME else (SA, AS)[k & 1]
        return eo == oo and es in (U, os_)
    if k >= 12:
        return False
    fwd = (k - 6) % 2 == 0
    if k < 10 and eo != SAME and k >= 8:
        fwd = not fwd
    return es in ((U, S) if fwd else (U, A))


def library_compat_mask(lib_format):
    """csrc/libdetfmt.h's ld_compat_mask: bit k set iff the format accepts kind k"""
    return sum(1 << k for k in range(len(LIBDET_KINDS)) if kind_compatible(lib_format, k))


def library_kinds_host(hits, offsets, *, paired_library, max_read_occs=200, allow_dovetail=False, remaining_votes=0, expected=None, stats=None):
    """The statement of the library-format tally (csrc/libdetfmt.h restated in numpy; what sfgpu_hits_library_kinds is judged by).
    hits: HIT_DTYPE records in CSR form over the reads (offsets[R + 1]).  A read without a record counts in `reads` only; one with more
    than max_read_occs in `reads_over_occs` and nothing else; any other in `reads_mapped`, its records in records_kind (per
    record_kinds_host), the read in reads_kind[k] where all its records are of kind k, else in reads_mixed, and -- with `expected`, a
    library format -- in reads_compatible iff one of its kinds is compatible (kind_compatible).  A mapped read votes iff all its
    records are of one kind and that is ISF .. MSR (paired_library) or SF / SR (single end); the first remaining_votes voters in read
    order are counted in votes_kind / votes.  The counters are added to `stats` (a dict as returned; None: zeros).
    -> (remaining_votes, stats dict of LIBDET_STATS: the *_kind entries lists in the order of LIBDET_KINDS)"""
    off = np.asarray(offsets).astype(np.int64)
    out = _libdet_stats(stats)
    R, K = max(len(off) - 1, 0), len(LIBDET_KINDS)
    remaining = int(remaining_votes)
    if R == 0:
        return remaining, out
    kinds = record_kinds_host(np.ascontiguousarray(hits, dtype=HIT_DTYPE)[: off[-1]], allow_dovetail).astype(np.int64)
    n = np.diff(off)
    over = n > int(max_read_occs)
    mapped = (n > 0) & ~over
    read_of = np.repeat(np.arange(R), n)
    mask = np.zeros(R, np.int64)
    np.bitwise_or.at(mask, read_of, 1 << kinds)
    mask[~mapped] = 0
    single = mapped & ((mask & (mask - 1)) == 0)
    read_kind = np.zeros(R, np.int64)
    read_kind[single] = np.log2(mask[single]).astype(np.int64)
    voting = 0x3F if paired_library else (1 << 10 | 1 << 11)
    voters = np.nonzero(single & ((mask & voting) != 0))[0][:max(remaining, 0)]
    compat = library_compat_mask(expected) if expected is not None else 0
    add = dict(reads=R, reads_mapped=int(mapped.sum()), reads_over_occs=int(over.sum()), reads_mixed=int((mapped & ~single).sum()),
               reads_compatible=int((mapped & ((mask & compat) != 0)).sum()), votes=len(voters),
               records_kind=np.bincount(kinds[mapped[read_of]], minlength=K).tolist(), reads_kind=np.bincount(read_kind[single], minlength=K).tolist(),
               votes_kind=np.bincount(read_kind[voters], minlength=K).tolist())
    for k, v in add.items():
        out[k] = [a + b for a, b in zip(out[k], v)] if isinstance(v, list) else out[k] + v
    return remaining - len(voters), out


def decide_library_format(votes, paired, min_fraction=0.7, min_votes=200):
    """csrc/libdetfmt.h's DECIDE over the votes of library_kinds (the 13 votes_kind counts, or a stats dict that holds them), in
    integers.  Paired: T = ISF + ISR, A = OSF + OSR, M = MSF + MSR; fewer than min_votes of them (or none): undetermined.  The
    orientation is the largest of T, A, M, ties in that order; with s its *SF count and n its sum the library is sense (ISF / OSF /
    MSF) iff 1000 s >= permille n, antisense (ISR / OSR / MSR) iff 1000 (n - s) >= permille n, else unstranded (IU / OU / MU).  Single
    end: the same with s = SF, n = SF + SR (SF / SR / U).  permille = int(round(min_fraction * 1000)), 501 .. 1000 (else ValueError).
    The default 0.7 is the customary threshold of other tools; nobody has measured it on real libraries here.  min_votes 200: at
    p = 0.5 a 70 % majority of 200 votes lies 5.6 sigma out, so an unstranded library is not called stranded by chance.
    -> (a name of LIBRARY_FORMATS or None where undetermined, detail dict: votes, orientation votes, sense, total, permille, min_votes)"""
    permille = _libdet_permille(min_fraction)
    v = [int(x) for x in (votes["votes_kind"] if isinstance(votes, dict) else votes)]
    if len(v) != len(LIBDET_KINDS):
        raise ValueError(f"{len(v)} vote counts, not one for each of the {len(LIBDET_KINDS)} kinds")
    min_votes = int(min_votes)
    if paired:
        inward, outward, matching = v[0] + v[1], v[2] + v[3], v[4] + v[5]
        total = inward + outward + matching
        detail = dict(votes=total, inward=inward, outward=outward, matching=matching)
        if inward >= outward and inward >= matching:
            orientation, s, n = TOWARD, v[0], inward
        elif outward >= matching:
            orientation, s, n = AWAY, v[2], outward
        else:
            orientation, s, n = SAME, v[4], matching
    else:
        orientation, s, n = NONE, v[10], v[10] + v[11]
        total = n
        detail = dict(votes=total)
    detail.update(sense=s, total=n, permille=permille, min_votes=min_votes)
    if total < min_votes or total == 0:
        return None, detail
    one_mate = orientation in (SAME, NONE)
    strand = U
    if 1000 * s >= permille * n:
        strand = S if one_mate else SA
    elif 1000 * (n - s) >= permille * n:
        strand = A if one_mate else AS
    return _FORMAT_NAMES[(1 if paired else 0, orientation, strand)], detail


def library_kinds(hits, offsets, *, paired_library, max_read_occs=200, allow_dovetail=False, remaining_votes=0, expected=None, stats=None, device="cuda"):
    """The library formats a batch's records show, tallied on the device (sfgpu_hits_library_kinds; the rule is library_kinds_host's,
    argument for argument).  hits / offsets: device tensors as QuasiIndex.map_reads returns them (or host arrays).  With
    remaining_votes == 0 no vote is looked for.  -> (remaining_votes, stats dict of LIBDET_STATS)"""
    dev = hits.device if isinstance(hits, torch.Tensor) and hits.is_cuda else torch.device(device)
    d_hits, d_off = _device_hits(hits, offsets, dev)
    R = int(d_off.numel()) - 1
    if R < 0:
        raise ValueError("hit offsets hold at least one entry")
    fmt = _format_triple(expected) if expected is not None else (0, 0, 0)
    o = _lib.LibdetOpts(int(max_read_occs), int(bool(paired_library)), int(bool(allow_dovetail)), int(expected is not None), _lib.LibFmt(fmt[0], fmt[1], fmt[2], 0))
    st = _lib.LibdetStats()
    for k, v in _libdet_stats(stats).items():
        if k.endswith("_kind"):
            getattr(st, k)[:] = v
        else:
            setattr(st, k, v)
    rem = C.c_int64(int(remaining_votes))
    with torch.cuda.device(dev):
        torch.cuda.current_stream().synchronize()
        _lib.check(_lib.lib().sfgpu_hits_library_kinds(_lib.ptr(d_hits), _lib.ptr(d_off), R, C.byref(o), C.byref(rem), C.byref(st), _lib.current_stream_ptr()))
    return int(rem.value), st.as_dict()


COVERAGE_STATS = ("reads", "records", "lines", "intervals", "empty_intervals", "bases_added")
COVERAGE_RESULT = ("runs", "bases_covered", "bases_total", "residue")
COV_ONE = 1 << 32
COV_MAX_LINES = (1 << 32) - 1


def coverage_weight(p):
    """csrc/coverfmt.h's WEIGHT of a posterior 0 <= p <= 1: trunc(p 2^32); the product is a scaling by a power of two, hence exact"""
    return int(p * 4294967296.0)


def coverage_host(ref_len, batches, *, finish=True):
    """The statement of the coverage pass (csrc/coverfmt.h restated; what sfgpu_cov_* are judged by).  ref_len: the transcripts'
    lengths; batches: an iterable of (hits, offsets, p, alignments) -- HIT_DTYPE records in CSR form over the reads, the posterior of
    every record (float64) or None for the uniform weight floor(2^32 / n) of a read with n records, and (pos, op_off, ops) as
    align_hits_host returns them (two slots a record) or None for the recorded diagonal.  Transcript t owns len_t + 1 slots of one
    uint64 array from off_t + t on; a line (line 0: pos, read_len; line 1 of a mate_status == 3 record: mate_pos, mate_len) adds
    q = trunc(p 2^32) at the start of each of its intervals, clipped to the transcript, and takes it off at the end; an inclusive
    scan modulo 2^64 gives the sums; a run is a maximal stretch of one transcript's bases with one nonzero sum.
    -> (runs = (tid uint32[], start uint32[], end uint32[], sum uint64[]), summary = (CoveredFraction, MeanDepth, MaxDepth float64[M]),
        stats dict of COVERAGE_STATS + COVERAGE_RESULT).  ValueError naming the lowest record of a batch whose tid is not a
    transcript, else the lowest whose p is NaN, negative or above 1, or saying that the lines would reach 2^32; nothing of that batch
    is added then."""
    ref_len = np.ascontiguousarray(ref_len, dtype=np.uint32)
    M = len(ref_len)
    base = np.zeros(M + 1, np.int64)
    np.cumsum(ref_len.astype(np.int64) + 1, out=base[1:])
    slot = np.zeros(int(base[M]), np.uint64)
    stats = dict.fromkeys(COVERAGE_STATS + COVERAGE_RESULT, 0)
    for hits, offsets, p, aln in batches:
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        off = np.asarray(offsets).astype(np.int64)
        n_rec = int(off[-1]) if len(off) else 0
        hits = hits[:n_rec]
        bad = np.nonzero(hits["tid"] >= M)[0]
        if len(bad):
            raise ValueError(f"record {int(bad[0])} names transcript >= {M}")
        if p is not None:
            p = np.ascontiguousarray(p, dtype=np.float64)[:n_rec]
            with np.errstate(invalid="ignore"):
                bad = np.nonzero(~((p >= 0) & (p <= 1)))[0]
            if len(bad):
                raise ValueError(f"the posterior of record {int(bad[0])} is NaN, negative or above 1")
            q = (p * 4294967296.0).astype(np.uint64)
        else:
            sizes = np.diff(off) if len(off) else np.zeros(0, np.int64)
            q = np.repeat(COV_ONE // np.maximum(sizes, 1), sizes).astype(np.uint64)
        paired = hits["mate_status"] == 3
        lines = n_rec + int(paired.sum())
        if stats["lines"] + lines > COV_MAX_LINES:
            raise ValueError(f"{lines} lines more would bring the total to 2^32 or beyond")
        stats["reads"] += max(len(off) - 1, 0)
        stats["records"] += n_rec
        stats["lines"] += lines
        tid = hits["tid"].astype(np.int64)
        len_t = ref_len[tid].astype(np.int64) if n_rec else np.zeros(0, np.int64)
        if aln is None:                                    # the recorded diagonal: line 0 of every record, line 1 of the pairs
            rec = np.concatenate([np.arange(n_rec), np.nonzero(paired)[0]])
            a = np.concatenate([hits["pos"].astype(np.int64), hits["mate_pos"].astype(np.int64)[paired]])
            b = a + np.concatenate([hits["read_len"].astype(np.int64), hits["mate_len"].astype(np.int64)[paired]])
        else:                                              # the covering words of every line's slot, walked from its position
            a_pos, a_off, a_ops = (np.asarray(x).astype(np.int64) for x in aln)
            if len(a_pos) != 2 * n_rec or len(a_off) != 2 * n_rec + 1:
                raise ValueError(f"alignments: expected {2 * n_rec} positions and {2 * n_rec + 1} offsets")
            a_ops = a_ops[:int(a_off[-1])] & 0xFFFFFFFF
            n, op = a_ops >> 4, a_ops & 15
            covers, advances = np.isin(op, (0, 7, 8)), np.isin(op, (0, 7, 8, 2, 3))
            slot_of = np.repeat(np.arange(2 * n_rec), np.diff(a_off))
            before = np.cumsum(np.where(advances, n, 0)) - np.where(advances, n, 0)          # the bases advanced before each word ...
            x = a_pos[slot_of] + before - before[np.minimum(a_off[:-1], max(len(before) - 1, 0))][slot_of] if len(a_ops) else np.zeros(0, np.int64)
            is_line = ((slot_of & 1) == 0) | paired[slot_of >> 1]
            sel = covers & is_line
            rec, a, b = slot_of[sel] >> 1, x[sel], x[sel] + n[sel]
        lo, hi = np.maximum(a, 0), np.minimum(b, len_t[rec])
        ok = lo < hi
        at, w = base[tid[rec]][ok], q[rec][ok]
        np.add.at(slot, at + lo[ok], w)
        np.subtract.at(slot, at + hi[ok], w)
        stats["intervals"] += int(ok.sum())
        stats["empty_intervals"] += int((~ok).sum())
        stats["bases_added"] += int((hi[ok] - lo[ok]).sum())
    if not finish:
        return slot, stats
    sums = np.cumsum(slot, dtype=np.uint64)
    r_tid, r_start, r_end, r_sum = [], [], [], []
    frac, mean, maxd = np.zeros(M), np.zeros(M), np.zeros(M)
    for t in range(M):
        n = int(ref_len[t])
        s = sums[int(base[t]):int(base[t]) + n]
        stats["residue"] += int(sums[int(base[t]) + n] != 0)
        if n == 0:
            continue
        change = np.nonzero(np.concatenate([[True], s[1:] != s[:-1]]))[0]
        ends = np.concatenate([change[1:], [n]])
        keep = s[change] != 0
        r_tid.append(np.full(int(keep.sum()), t, np.uint32))
        r_start.append(change[keep].astype(np.uint32))
        r_end.append(ends[keep].astype(np.uint32))
        r_sum.append(s[change][keep])
        covered = int((s != 0).sum())
        total = int((s & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64)) + (int((s >> np.uint64(32)).sum(dtype=np.uint64)) << 32)      # 128 bits
        stats["bases_covered"] += covered
        frac[t], mean[t], maxd[t] = covered / n, float(total // n) * 2.0 ** -32, float(int(s.max())) * 2.0 ** -32
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)      # noqa: E731
    runs = (cat(r_tid, np.uint32), cat(r_start, np.uint32), cat(r_end, np.uint32), cat(r_sum, np.uint64))
    stats["runs"] = len(runs[0])
    stats["bases_total"] = int(ref_len.astype(np.int64).sum())
    return runs, (frac, mean, maxd), stats


def gc_prefix(seq, seq_off, ref_len):
    """Transcript::GCCount_ of every transcript (include/Transcript.hpp:183-196), laid out like `seq`: int32 device
    tensor of seq.numel() entries (4 bytes per base) -- what sample_bias reads for the fragment-GC samples."""
    out = torch.zeros(seq.numel(), dtype=torch.int32, device=seq.device)
    so = seq_off.to(torch.int64).contiguous()
    with torch.cuda.device(seq.device):
        _lib.check(_lib.lib().sfgpu_gc_prefix(_lib.ptr(seq), _lib.ptr(so), _lib.ptr(ref_len), int(ref_len.numel()), _lib.ptr(out),
                                              _lib.current_stream_ptr()))
        torch.cuda.current_stream().synchronize()
    return out


def sample_bias(hits, hit_offsets, lib_format, seq, seq_off, ref_len, *, read_bias=None, remaining_bias_samples=0,
                observed_gc=None, gc_prefix_table=None, gc_size_samp=1, paired_library=None, allow_orphans=False,
                max_read_occs=200, max_frag_len=1000, device="cuda"):
    """The bias / GC samples the hit loop collects (src/SailfishQuantify.cpp:270-287, 375-389, 559-581) over the reads and
    hits that survive filter_hits' cuts.  read_bias (int32 device tensor [4096]) and observed_gc ([101]) are updated in
    place when given.  Returns (remaining_bias_samples, n_bias_sampled, n_gc_sampled)."""
    dev = torch.device(device)
    fmt = LIBRARY_FORMATS[lib_format.upper()] if isinstance(lib_format, str) else tuple(lib_format)
    if paired_library is None:
        paired_library = fmt[0] == 1
    d_hits, d_off = _device_hits(hits, hit_offsets, dev)
    R = int(d_off.numel()) - 1
    o = _lib.FilterOpts(int(max_read_occs), int(max_frag_len), int(bool(paired_library)), int(not allow_orphans), 0, 0, 0,
                        _lib.LibFmt(int(fmt[0]), int(fmt[1]), int(fmt[2]), 0))
    so = seq_off.to(torch.int64).contiguous()
    rem = C.c_int64(int(remaining_bias_samples))
    sp = _lib.BiasSampler(_lib.ptr(seq).value, _lib.ptr(so).value, _lib.ptr(ref_len).value,
                          None if read_bias is None else _lib.ptr(read_bias).value, C.pointer(rem),
                          None if observed_gc is None else _lib.ptr(observed_gc).value,
                          None if gc_prefix_table is None else _lib.ptr(gc_prefix_table).value, 0, 0, int(gc_size_samp), 0)
    with torch.cuda.device(dev):
        torch.cuda.current_stream().synchronize()
        _lib.check(_lib.lib().sfgpu_sample_bias(_lib.ptr(d_hits), _lib.ptr(d_off), R, C.byref(o), C.byref(sp), _lib.current_stream_ptr()))
    return int(rem.value), int(sp.n_bias_sampled), int(sp.n_gc_sampled)


GENOME_COVERAGE_STATS = ("n_pieces", "n_events", "n_keys", "n_runs", "bases_covered", "runs_unplaced", "bases_unplaced", "bases_off_model",
                         "transcripts_placed", "transcripts_length_mismatch")


def coverage_genome_host(runs, placement, ref_len=None, with_distinct=False):
    """The statement of the projection onto the chromosomes (csrc/covgfmt.h restated with Python integers; what sfgpu_covg_* are judged
    by).  runs: coverage_host's (tid, start, end, sum); placement: genes.ExonModel.for_names' result (status, chrom, strand, exon_off,
    exon_start, exon_len -- blocks in transcript order).  A run of a placed transcript is cut at its blocks; a piece [lo, hi) on
    chromosome c adds +sum at key c << 32 | lo and -sum at c << 32 | hi, modulo 2^64; keys whose delta is 0 disappear; the running sum
    over the ascending keys holds from a key to the next; the stretches of nonzero sum are the runs.  ref_len (the transcripts' lengths)
    is only compared with the blocks' total for `transcripts_length_mismatch` (0 without it).  with_distinct=True adds two counts the
    device's grids are sized by and its result does not carry: `n_distinct`, the keys before those of delta 0 are dropped, and `n_long`,
    the runs of more than 8 pieces.
    -> (runs = (chrom uint32[], start uint32[], end uint32[], sum uint64[]), stats dict of GENOME_COVERAGE_STATS)"""
    status, chrom, strand, exon_off, exon_start, exon_len = (np.asarray(getattr(placement, k)) for k in ("status", "chrom", "strand", "exon_off", "exon_start", "exon_len"))
    M, mask = len(status), (1 << 64) - 1
    eo = [int(x) for x in exon_off]
    gs, ln = [int(x) for x in exon_start], [int(x) for x in exon_len]
    st = dict.fromkeys(GENOME_COVERAGE_STATS, 0)
    total = [sum(ln[eo[t]:eo[t + 1]]) for t in range(M)]
    for t in range(M):
        if status[t] == 0:
            st["transcripts_placed"] += 1
            st["transcripts_length_mismatch"] += int(ref_len is not None and total[t] != int(ref_len[t]))
    delta, n_long = {}, 0
    for t, a, b, s in zip(*(np.asarray(x).tolist() for x in runs)):
        if status[t] != 0:
            st["runs_unplaced"] += 1
            st["bases_unplaced"] += b - a
            continue
        if b > total[t]:
            st["bases_off_model"] += b - max(a, total[t])
            b = total[t]
        c, toff, before = int(chrom[t]) << 32, 0, st["n_pieces"]
        for e in range(eo[t], eo[t + 1]):
            a1, b1 = max(a, toff), min(b, toff + ln[e])
            if a1 < b1:
                lo, hi = (gs[e] + a1 - toff, gs[e] + b1 - toff) if strand[t] > 0 else (gs[e] + ln[e] - (b1 - toff), gs[e] + ln[e] - (a1 - toff))
                delta[c | lo] = (delta.get(c | lo, 0) + s) & mask
                delta[c | hi] = (delta.get(c | hi, 0) - s) & mask
                st["n_pieces"] += 1
            toff += ln[e]
        n_long += st["n_pieces"] - before > 8
    st["n_events"] = 2 * st["n_pieces"]
    out, acc = ([], [], [], []), 0
    for key in sorted(delta):
        if delta[key] == 0:
            continue
        st["n_keys"] += 1
        if acc:
            out[2].append(key & 0xFFFFFFFF)
        acc = (acc + delta[key]) & mask
        if acc:
            out[0].append(key >> 32); out[1].append(key & 0xFFFFFFFF); out[3].append(acc)
    if len(out[2]) != len(out[0]):
        raise ValueError("a chromosome's deltas do not sum to 0")
    st["n_runs"] = len(out[0])
    st["bases_covered"] = sum(e - s for s, e in zip(out[1], out[2]))
    if with_distinct:
        st["n_distinct"], st["n_long"] = len(delta), n_long
    return (np.array(out[0], np.uint32), np.array(out[1], np.uint32), np.array(out[2], np.uint32), np.array(out[3], np.uint64)), st


GENOME_ALN_STATS = ("records_in", "records_out", "records_unplaced", "records_unalignable", "records_off_range", "reads_emptied", "lines", "lines_spliced",
                    "n_operations", "lines_reversed", "columns_beyond_model", "words_in", "words_out")
GALN_MAX_END = (1 << 31) - 1                            # a line's interval ends at or below it
GALN_MAX_OP = 1 << 28                                   # an operation is shorter
_MD_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def md_reverse(md):
    """csrc/galnfmt.h's MD of a line on a - transcript: the tokens num (letter | ^letters) num ... in reverse order, a letter complemented
    (A<->T, C<->G, everything else as it is), a deletion's letters reversed and complemented: b"5^AC0T3" -> b"3A0^GT5" """
    tokens, i, n = [], 0, len(md)
    while i < n:
        j = i + 1
        if 48 <= md[i] <= 57:
            while j < n and 48 <= md[j] <= 57:
                j += 1
            tokens.append(md[i:j])
        elif md[i] == 94:
            while j < n and not 48 <= md[j] <= 57 and md[j] != 94:
                j += 1
            tokens.append(b"^" + md[i + 1:j].translate(_MD_COMP)[::-1])
        else:
            tokens.append(md[i:j].translate(_MD_COMP))
        i = j
    return b"".join(reversed(tokens))


def _galn_line_host(words, x0, blocks, strand):
    """One line by the rule of csrc/galnfmt.h, column by column: words = its transcript CIGAR, x0 = POS - 1 >= 0, blocks = the
    transcript's [(gs, len)] in transcript order (at least one) -> (the words in transcript order, lo, hi, N operations, columns beyond
    the model, whether an N is too long)"""
    toff = [0]
    for _, ln in blocks:
        toff.append(toff[-1] + ln)
    L, last = toff[-1], len(blocks) - 1
    out, x, b, prev, first, n_N, beyond, too_long = [], x0, 0, None, None, 0, 0, False
    for w in words:
        n, op = w >> 4, w & 15
        if op not in _MATCH_OPS + _DEL_OPS or n == 0:
            out.append(w)
            continue
        cur = 0
        for _ in range(n):
            while b < last and x >= toff[b + 1]:
                b += 1
            d = x - toff[b]
            g = blocks[b][0] + d if strand > 0 else blocks[b][0] + blocks[b][1] - 1 - d
            if prev is not None and abs(g - prev) > 1:      # the column does not touch the one before it: a junction lies between them
                if cur:
                    out.append(cur << 4 | op)
                    cur = 0
                gap = abs(g - prev) - 1
                out.append(gap << 4 | 3)
                n_N += 1
                too_long |= gap >= GALN_MAX_OP
            first = g if first is None else first
            beyond += x >= L
            prev, cur, x = g, cur + 1, x + 1
        out.append(cur << 4 | op)
    lo, hi = (first, prev + 1) if strand > 0 else (prev, first + 1)
    return out, lo, hi, n_N, beyond, too_long


def project_alignments_host(hits, offsets, placement, alignments=None, tags=None):
    """The statement of the projection of a batch onto the genome (csrc/galnfmt.h restated in plain loops with Python integers; what
    sfgpu_galn_project is judged by).  hits / offsets: HIT_DTYPE records in CSR form over the reads; placement: genes.ExonModel.for_names'
    result for the transcripts the records name; alignments: what align_hits / align_hits_host returned for the same records (pos, nm,
    op_off, ops, ...) or None for the writer's <clip>S<match>M; tags: what md_tags / md_tags_host returned (nm, md_off, md, ...) or None.
    A record is kept iff its transcript is placed (status 0 and at least one block), every line -- line 0, and line 1 of a mate_status
    3 record -- has a reference column (an M = X D N word of length > 0), and every line starts at x0 >= 0, projects into
    [0, 2^31 - 1] and needs no N of 2^28 bases or more; the first failing test counts it as records_unplaced, records_unalignable or
    records_off_range.  A kept line's reference columns are placed in the blocks (beyond the blocks' total length the last block goes
    on: columns_beyond_model); where two consecutive columns do not touch on the chromosome the word is cut and <gap>N put between
    them; on a - transcript the words are reversed, fwd / mate_fwd inverted and the MD reversed (md_reverse).  The record takes tid =
    the chromosome id, pos / mate_pos = its lines' 0-based genome positions, frag_len of a pair = the span of both lines.
    -> (hits, offsets uint32[R + 1], alignments = (pos int32[2 n'], nm uint32[2 n'], op_off uint64[2 n' + 1], ops uint32[]),
        tags = (nm, md_off, md) or None, src_record uint32[n'], stats dict of GENOME_ALN_STATS); ValueError naming the lowest record
    whose tid is not a transcript of the placement."""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    off = np.asarray(offsets).astype(np.int64)
    n_rec = int(off[-1]) if len(off) else 0
    status, chrom, strand, exon_off, exon_start, exon_len = (np.asarray(getattr(placement, k)) for k in ("status", "chrom", "strand", "exon_off", "exon_start", "exon_len"))
    M = len(status)
    bad = np.nonzero(hits["tid"][:n_rec] >= M)[0]
    if len(bad):
        raise ValueError(f"record {int(bad[0])} names transcript >= {M}")
    host = lambda v, dt: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)).view(dt).reshape(-1)      # noqa: E731
    aln = tg = None
    if alignments is not None:
        aln = host(alignments[0], np.int32), host(alignments[1], np.uint32), host(alignments[2], np.uint64), host(alignments[3], np.uint32)
        if len(aln[0]) != 2 * n_rec or len(aln[2]) != 2 * n_rec + 1:
            raise ValueError(f"an alignment of {len(aln[0])} slots for {n_rec} records (two slots a record)")
    if tags is not None:
        tg = host(tags[0], np.uint32), host(tags[1], np.uint64), host(tags[2], np.uint8).tobytes()
        if len(tg[0]) != 2 * n_rec or len(tg[1]) != 2 * n_rec + 1:
            raise ValueError(f"tags of {len(tg[0])} slots for {n_rec} records (two slots a record)")
    st = dict.fromkeys(GENOME_ALN_STATS, 0)
    o_hits, o_off, o_pos, o_nm, o_cnt, o_ops, t_nm, t_cnt, t_md, src = [], [0], [], [], [], [], [], [], [], []
    for r in range(len(off) - 1):
        for i in range(int(off[r]), int(off[r + 1])):
            h = hits[i]
            t, two = int(h["tid"]), int(h["mate_status"]) == 3
            st["records_in"] += 1
            blocks = [(int(exon_start[e]), int(exon_len[e])) for e in range(int(exon_off[t]), int(exon_off[t + 1]))]
            if status[t] != 0 or not blocks:
                st["records_unplaced"] += 1
                continue
            lines = []
            for j in range(2 if two else 1):
                s = 2 * i + j
                if aln is not None:
                    words, x0 = [int(w) for w in aln[3][int(aln[2][s]):int(aln[2][s + 1])]], int(aln[0][s])
                else:
                    pos, length = (int(h["mate_pos"]), int(h["mate_len"])) if j else (int(h["pos"]), int(h["read_len"]))
                    if pos >= 0:
                        words, x0 = [length << 4], pos
                    elif -pos < length:
                        words, x0 = [-pos << 4 | CIGAR_S, (length + pos) << 4], 0
                    else:
                        words, x0 = [], 0
                lines.append((words, x0))
            if any(not any((w & 15) in _MATCH_OPS + _DEL_OPS and w >> 4 for w in words) for words, _ in lines):
                st["records_unalignable"] += 1
                continue
            walked = [None if x0 < 0 else _galn_line_host(words, x0, blocks, int(strand[t])) for words, x0 in lines]
            if any(w is None or w[1] < 0 or w[2] > GALN_MAX_END or w[5] for w in walked):
                st["records_off_range"] += 1
                continue
            st["records_out"] += 1
            rev = int(strand[t]) < 0
            rec = h.copy()
            rec["tid"], rec["pos"] = int(chrom[t]), walked[0][1]
            if two:
                rec["mate_pos"] = walked[1][1]
                rec["frag_len"] = max(walked[0][2], walked[1][2]) - min(walked[0][1], walked[1][1])
            if rev:
                rec["fwd"], rec["mate_fwd"] = int(not h["fwd"]), int(not h["mate_fwd"])
            o_hits.append(rec)
            src.append(i)
            for j in range(2):
                s = 2 * i + j
                if j == 1 and not two:
                    o_pos.append(0); o_nm.append(0); o_cnt.append(0); t_nm.append(0); t_cnt.append(0)
                    continue
                out, lo, _, n_N, beyond, _ = walked[j]
                st["lines"] += 1
                st["lines_spliced"] += int(n_N > 0)
                st["n_operations"] += n_N
                st["lines_reversed"] += int(rev)
                st["columns_beyond_model"] += beyond
                st["words_in"] += len(lines[j][0])
                st["words_out"] += len(out)
                o_pos.append(lo)
                o_nm.append(int(aln[1][s]) if aln is not None else 0)
                o_cnt.append(len(out))
                o_ops += out[::-1] if rev else out
                if tg is not None:
                    md = tg[2][int(tg[1][s]):int(tg[1][s + 1])]
                    t_nm.append(int(tg[0][s])); t_cnt.append(len(md))
                    t_md.append(md_reverse(md) if rev else md)
        st["reads_emptied"] += int(off[r + 1] > off[r] and len(o_hits) == o_off[-1])
        o_off.append(len(o_hits))
    csr = lambda counts: np.concatenate([[0], np.cumsum(np.array(counts, np.uint64), dtype=np.uint64)]).astype(np.uint64)      # noqa: E731
    out_hits = np.array(o_hits, dtype=HIT_DTYPE) if o_hits else np.zeros(0, HIT_DTYPE)
    out_aln = (np.array(o_pos, np.int32), np.array(o_nm, np.uint32), csr(o_cnt), np.array(o_ops, np.uint32))
    out_tags = (np.array(t_nm, np.uint32), csr(t_cnt), np.frombuffer(b"".join(t_md), np.uint8)) if tg is not None else None
    return out_hits, np.array(o_off, np.uint32), out_aln, out_tags, np.array(src, np.uint32), st


class GenomeAlignments:
    """GenomeAlignments(placement, device): the exon model on the device for project_alignments (sfgpu_galn_open: validated by the
    rule of the genome coverage's model, an SfgpuError naming the lowest offending transcript otherwise).  close() frees it; usable as
    a context manager.  `stats` sums the counters of the batches projected through it."""

    def __init__(self, placement, device="cuda"):
        self._L, self._h = _lib.lib(), None
        self.device = torch.device(device)
        dev = lambda a, dt, bits: torch.from_numpy(np.ascontiguousarray(a, dt).view(bits).copy()).to(self.device)      # noqa: E731
        model = (dev(placement.status, np.uint8, np.uint8), dev(placement.chrom, np.int32, np.int32), dev(placement.strand, np.int8, np.int8),
                 dev(placement.exon_off, np.uint64, np.int64), dev(placement.exon_start, np.uint32, np.int32), dev(placement.exon_len, np.uint32, np.int32))
        self.M, self.n_chrom = int(model[0].numel()), int(placement.n_chrom)
        if model[1].numel() != self.M or model[2].numel() != self.M or model[3].numel() != self.M + 1:
            raise ValueError(f"the placement is not one of {self.M} transcripts")
        E = int(placement.exon_off[-1])
        if model[4].numel() != E or model[5].numel() != E:
            raise ValueError(f"the placement's offsets end at {E} but it holds {model[4].numel()} block starts and {model[5].numel()} lengths")
        self.stats = dict.fromkeys(GENOME_ALN_STATS, 0)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()
            _lib.check(self._L.sfgpu_galn_open(C.byref(h), *(_lib.ptr(t) if t.numel() else None for t in model[:3]), _lib.ptr(model[3]),
                                               *(_lib.ptr(t) if t.numel() else None for t in model[4:]), self.M, self.n_chrom, _lib.current_stream_ptr()))
        self._h = h

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            with torch.cuda.device(self.device):
                self._L.sfgpu_galn_close(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001
            pass


def project_alignments(hits, offsets, placement, alignments=None, tags=None, *, device="cuda", _room=None):
    """project_alignments_host on the device (sfgpu_galn_project; csrc/genomealn.hip).  hits / offsets: a batch as map_reads returns it
    (device tensors) or numpy arrays; placement: genes.ExonModel.for_names' result, or a GenomeAlignments made of one (a run opens the
    model once); alignments / tags: what align_hits / md_tags returned for the same records, or None.  The words' room is sized at the
    words given plus two a slot (an ungapped line has at most two words), the MD's at the bytes given, and the call repeated once with the counts the library
    reports where they do not fit (_room = (words, MD bytes) overrides the first sizes: for tests).
    -> (hits uint8 tensor of HIT_DTYPE records, offsets int32[R + 1], alignments = (pos int32[2 n'], nm int32[2 n'], op_off int64[2 n' + 1],
        ops int32[]), tags = (nm int32[2 n'], md_off int64[2 n' + 1], md uint8[]) or None, src_record int32[n'], stats dict of
        GENOME_ALN_STATS): device tensors, the bits of the unsigned values."""
    own = not isinstance(placement, GenomeAlignments)
    g = GenomeAlignments(placement, device) if own else placement
    try:
        dev = g.device
        d_hits, d_off = _device_hits(hits, offsets, dev)
        R, n = int(d_off.numel()) - 1, d_hits.numel() // 24
        signed = {1: np.uint8, 4: np.int32, 8: np.int64}
        up = lambda v: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v).view(signed[v.dtype.itemsize]).copy())).to(dev).contiguous()      # noqa: E731
        some = lambda t, dt: t if t.numel() else torch.zeros(1, dtype=dt, device=dev)      # noqa: E731  (nothing at all: still "given")
        b = _lib.GalnBatch(_lib.ptr(d_hits) if n else None, _lib.ptr(d_off), max(R, 0), 0)
        keep, words_in, md_in = [d_hits, d_off], 0, 0
        if alignments is not None:
            a_pos, a_nm, a_off, a_ops = (up(alignments[i]) for i in range(4))
            if int(a_pos.numel()) != 2 * n or int(a_off.numel()) != 2 * n + 1 or int(a_nm.numel()) != 2 * n:
                raise ValueError(f"an alignment of {int(a_pos.numel())} slots for {n} records (two slots a record)")
            words_in = int(a_ops.numel())
            a_pos, a_nm, a_ops = some(a_pos, torch.int32), some(a_nm, torch.int32), some(a_ops, torch.int32)
            b.aln_pos, b.aln_op_off, b.aln_ops, b.aln_nm = _lib.ptr(a_pos), _lib.ptr(a_off), _lib.ptr(a_ops), _lib.ptr(a_nm)
            keep += [a_pos, a_nm, a_off, a_ops]
        if tags is not None:
            t_nm, t_off, t_md = (up(tags[i]) for i in range(3))
            if int(t_nm.numel()) != 2 * n or int(t_off.numel()) != 2 * n + 1:
                raise ValueError(f"tags of {int(t_nm.numel())} slots for {n} records (two slots a record)")
            md_in = int(t_md.numel())
            t_nm, t_md = some(t_nm, torch.int32), some(t_md, torch.uint8)
            b.tag_nm, b.tag_md_off, b.tag_md = _lib.ptr(t_nm), _lib.ptr(t_off), _lib.ptr(t_md)
            keep += [t_nm, t_off, t_md]
        o_hits = torch.zeros(max(n, 1) * 24, dtype=torch.uint8, device=dev)
        o_off = torch.zeros(R + 1, dtype=torch.int32, device=dev)
        o_pos, o_nm, o_tnm = (torch.zeros(max(2 * n, 1), dtype=torch.int32, device=dev) for _ in range(3))
        o_aoff, o_moff = (torch.zeros(2 * n + 1, dtype=torch.int64, device=dev) for _ in range(2))
        src = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        st, need_ops, need_md = _lib.GalnStats(), C.c_uint64(0), C.c_uint64(0)
        cap_ops, cap_md = (words_in + 4 * n, md_in) if _room is None else (int(_room[0]), int(_room[1]))
        with torch.cuda.device(dev):
            torch.cuda.current_stream().synchronize()
            for attempt in range(2):
                ops = torch.zeros(max(cap_ops, 1), dtype=torch.int32, device=dev)
                md = torch.zeros(max(cap_md, 1), dtype=torch.uint8, device=dev)
                o = _lib.GalnOut(_lib.ptr(o_hits), _lib.ptr(o_off), _lib.ptr(o_pos), _lib.ptr(o_nm), _lib.ptr(o_aoff), _lib.ptr(ops), cap_ops,
                                 _lib.ptr(o_tnm), _lib.ptr(o_moff), _lib.ptr(md), cap_md, _lib.ptr(src))
                rc = g._L.sfgpu_galn_project(g._h, C.byref(b), C.byref(o), C.byref(need_ops), C.byref(need_md), C.byref(st), _lib.current_stream_ptr())
                if rc != _lib.ERR_RANGE or attempt or (need_ops.value <= cap_ops and need_md.value <= cap_md):
                    break
                cap_ops, cap_md = max(cap_ops, int(need_ops.value)), max(cap_md, int(need_md.value))
            _lib.check(rc)
        del keep
        stats = {k: int(getattr(st, k)) for k in GENOME_ALN_STATS}
        for k, v in stats.items():
            g.stats[k] += v
        m = stats["records_out"]
        out_tags = (o_tnm[:2 * m], o_moff[:2 * m + 1], md[:int(need_md.value)]) if tags is not None else None
        return o_hits[:24 * m], o_off, (o_pos[:2 * m], o_nm[:2 * m], o_aoff[:2 * m + 1], ops[:int(need_ops.value)]), out_tags, src[:m], dict(stats, project_ms=st.project_ms)
    finally:
        if own:
            g.close()
