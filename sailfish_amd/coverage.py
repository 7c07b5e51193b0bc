"""Posterior-weighted transcript coverage as bedGraph, from the device -- what `rsem-bam2wig` makes of a ZW-tagged BAM, without the
BAM, the sort and the CPU pass:

    name \\t start \\t end \\t %g(depth) \\n        one row per run, 0-based and half open, no header line

A run is a maximal stretch of one transcript's bases with the same depth; runs of depth 0 are left out.  CoverageDevice keeps ONE
uint64 array on the device over all batches of a run (sfgpu_cov_*: 8 bytes per base and transcript), adds every batch's lines with
64-bit integer atomics and, at the end, scans, finds the runs and formats the rows there.  The rule is csrc/coverfmt.h's,
hits.coverage_host is its statement and coverage_text_host the statement of the file's bytes: what tools and tests compare against."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib, quantfile
from .hits import COVERAGE_STATS, _device_hits

SUMMARY_HEADER = b"Name\tLength\tCoveredFraction\tMeanDepth\tMaxDepth\n"


def coverage_text_host(names, runs):
    """The bytes of the bedGraph file for coverage_host's runs (tid, start, end, sum); names as str or bytes, one "%g" at a time"""
    enc = [n.encode("utf-8") if isinstance(n, str) else bytes(n) for n in names]
    tid, start, end, total = runs
    return b"".join(enc[int(t)] + b"\t%d\t%d\t%s\n" % (int(a), int(b), ("%g" % (float(int(s)) * 2.0 ** -32)).encode())
                    for t, a, b, s in zip(tid.tolist(), start.tolist(), end.tolist(), total.tolist()))


def genome_text_host(chrom_names, runs):
    """The bytes of the genome bedGraph file for hits.coverage_genome_host's runs (chrom, start, end, sum): coverage_text_host's rows with
    the chromosomes' names in place of the transcripts'"""
    return coverage_text_host(chrom_names, runs)


def summary_text_host(names, ref_len, summary):
    """The bytes of aux/coverage_summary.tsv for coverage_host's summary: the header and quantfile.format_rows over the three columns"""
    return SUMMARY_HEADER + quantfile.format_rows(names, ref_len, *summary)


def _device_names(names, dev):
    if isinstance(names, tuple) and len(names) == 2 and isinstance(names[0], torch.Tensor):
        return names[0].to(dev).contiguous(), names[1].to(dev).contiguous()
    b, o = quantfile.names_blob(names)
    return torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(dev), torch.from_numpy(o.view(np.int64).copy()).to(dev)


class CoverageDevice:
    """CoverageDevice(ref_len, device): the coverage of the transcripts of these lengths (a uint32 array or a 32-bit integer tensor),
    accumulated on `device`.
    add(hits, offsets, posteriors=None, alignments=None)   one batch: records and offsets as QuasiIndex.map_reads returns them (or
        host arrays); posteriors: float64, one per record (hits.posteriors' p), None for the uniform weight of a read's records;
        alignments: (pos, op_off, ops) of hits.align_hits for the same records, None for the recorded diagonal.  A batch that is
        refused (SfgpuError) leaves the state as it was.
    finish() -> the result dict (runs, bases_covered, bases_total, residue, state_bytes); nothing can be added afterwards
    runs() -> (tid int32, start int32, end int32, sum int64) device tensors (the bits of the unsigned values)
    summary() -> (CoveredFraction, MeanDepth, MaxDepth) float64 device tensors, one entry per transcript
    write(path_or_file, names, compress=False, chunk_bytes=0)   the bedGraph file, formatted on the device; compress=True: BGZF,
        encoded on the device; -> the write's result dict
    write_summary(path_or_file, names)   the header line and the rows of sfgpu_quant_write_text over the three columns
    `stats` sums the batches (COVERAGE_STATS).  close() frees the device array; usable as a context manager."""

    def __init__(self, ref_len, device="cuda"):
        self._L = _lib.lib()
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if isinstance(ref_len, torch.Tensor):
            if ref_len.is_floating_point() or ref_len.element_size() != 4:
                raise TypeError("ref_len: expected 32-bit integers")
            self.ref_len = ref_len.to(self.device).contiguous()
        else:
            self.ref_len = torch.from_numpy(np.ascontiguousarray(ref_len, np.uint32).view(np.int32).copy()).to(self.device)
        self.M = int(self.ref_len.numel())
        self.stats = dict.fromkeys(COVERAGE_STATS, 0)
        self.result = None
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()
            _lib.check(self._L.sfgpu_cov_open(C.byref(h), _lib.ptr(self.ref_len) if self.M else None, self.M, _lib.current_stream_ptr()))
        self._h = h

    def add(self, hits, offsets, posteriors=None, alignments=None):
        if self._h is None:
            raise ValueError("the coverage is closed")
        d_hits, d_off = _device_hits(hits, offsets, self.device)
        R, n = int(d_off.numel()) - 1, d_hits.numel() // 24
        if R < 0:
            raise ValueError("hit offsets hold at least one entry")
        p = None
        if posteriors is not None:
            p = (posteriors if isinstance(posteriors, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(posteriors, np.float64).copy()))
            p = p.to(self.device, torch.float64).contiguous()
            if p.numel() != n:
                raise ValueError(f"{p.numel()} posteriors for {n} records")
        aln = (None, None, None)
        if alignments is not None:
            pos, op_off, ops = alignments
            as_dev = lambda x, dt, bits: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dt).view(bits).copy())).to(self.device).contiguous()      # noqa: E731
            aln = (as_dev(pos, np.int32, np.int32), as_dev(op_off, np.uint64, np.int64), as_dev(ops, np.uint32, np.int32))
            if aln[0].numel() != 2 * n or aln[1].numel() != 2 * n + 1 or aln[0].element_size() != 4 or aln[1].element_size() != 8 or aln[2].element_size() != 4:
                raise ValueError(f"alignments: expected pos[{2 * n}] of 32 bits, op_off[{2 * n + 1}] of 64 bits and ops of 32 bits")
        st = _lib.CovStats()
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()
            _lib.check(self._L.sfgpu_cov_add(self._h, _lib.ptr(d_hits) if n else None, _lib.ptr(d_off), R, _lib.ptr(p) if p is not None and n else None,
                                             _lib.ptr(aln[0]) if aln[0] is not None and n else None, _lib.ptr(aln[1]) if aln[1] is not None and n else None,
                                             _lib.ptr(aln[2]) if aln[2] is not None and n and aln[2].numel() else None, C.byref(st), _lib.current_stream_ptr()))
        for k, v in st.as_dict().items():
            self.stats[k] += v
        return st.as_dict()

    def finish(self):
        if self._h is None:
            raise ValueError("the coverage is closed")
        res = _lib.CovResult()
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()
            _lib.check(self._L.sfgpu_cov_finish(self._h, C.byref(res), _lib.current_stream_ptr()))
        self.result = {k: int(getattr(res, k)) for k in ("n_runs", "bases_covered", "bases_total", "residue", "state_bytes")}
        self.result["runs"] = self.result.pop("n_runs")
        self.result["finish_ms"] = res.finish_ms
        return self.result

    def _finished(self):
        if self.result is None:
            self.finish()

    def runs(self):
        self._finished()
        n = self.result["runs"]
        tid, start, end = (torch.zeros(n, dtype=torch.int32, device=self.device) for _ in range(3))
        total = torch.zeros(n, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.sfgpu_cov_runs(self._h, *(_lib.ptr(t) if n else None for t in (tid, start, end, total))))
        return tid, start, end, total

    def summary(self):
        self._finished()
        cols = tuple(torch.zeros(self.M, dtype=torch.float64, device=self.device) for _ in range(3))
        with torch.cuda.device(self.device):
            _lib.check(self._L.sfgpu_cov_summary(self._h, *(_lib.ptr(t) if self.M else None for t in cols)))
        return cols

    def write(self, path_or_file, names, compress=False, chunk_bytes=0):
        self._finished()
        blob, off = _device_names(names, self.device)
        if off.numel() != self.M + 1:
            raise ValueError(f"{off.numel() - 1} names for {self.M} transcripts")
        args = (self._h, _lib.ptr(blob) if blob.numel() else None, _lib.ptr(off), int(chunk_bytes))
        return _write_rows(path_or_file, self.device, compress, chunk_bytes, _lib.CovResult(),
                           lambda sink, res: self._L.sfgpu_cov_write_text(*args, sink, None, C.byref(res), _lib.current_stream_ptr()),
                           lambda z, res: self._L.sfgpu_cov_write_bgzf(*args, z, C.byref(res), _lib.current_stream_ptr()))

    def write_summary(self, path_or_file, names):
        frac, mean, maxd = self.summary()
        own = isinstance(path_or_file, (str, bytes, os.PathLike))
        f = open(path_or_file, "wb") if own else path_or_file
        try:
            f.write(SUMMARY_HEADER)
            if self.M:
                names = names if not (isinstance(names, tuple) and isinstance(names[0], torch.Tensor)) else _device_names(names, self.device)
                return quantfile.write_rows(f, names, self.ref_len, frac, mean, maxd)
        finally:
            if own:
                f.close()

    def project(self, placement):
        """-> GenomeCoverageDevice: the runs projected through `placement` (genes.ExonModel.for_names of this coverage's transcripts)
        onto the chromosomes and summed per genomic base, on the device (sfgpu_covg_*)"""
        self._finished()
        return GenomeCoverageDevice(self, placement)

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            with torch.cuda.device(self.device):
                self._L.sfgpu_cov_close(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001
            pass


def _write_rows(f_or_path, device, compress, chunk_bytes, result, text_call, bgzf_call):
    """one bedGraph file through a sink (text_call(sink, result)) or the device's BGZF encoder (bgzf_call(handle, result))"""
    own = isinstance(f_or_path, (str, bytes, os.PathLike))
    f = open(f_or_path, "wb") if own else f_or_path
    raised = []

    def sink(addr, n, _user):
        try:                                   # nothing may unwind through the C frame
            f.write(memoryview((C.c_char * n).from_address(addr)))
            return 0
        except BaseException as e:             # noqa: BLE001  (re-raised below)
            raised.append(e)
            return 1

    try:
        with torch.cuda.device(device):
            torch.cuda.current_stream().synchronize()
            if not compress:
                rc = text_call(_lib.TEXT_SINK(sink), result)
            else:
                from . import gzfile
                z = gzfile.BgzfDeviceWriter(f, chunk_bytes=int(chunk_bytes))
                z._open(device)
                rc = bgzf_call(z._h, result)
                raised = z._raised
                z.close()
        if raised:
            raise raised[0]
        _lib.check(rc)
    finally:
        if own:
            f.close()
    return result.as_dict()


class GenomeCoverageDevice:
    """GenomeCoverageDevice(coverage, placement): a finished CoverageDevice's runs projected onto the chromosomes (csrc/covgfmt.h;
    hits.coverage_genome_host is the statement).  placement: genes.ExonModel.for_names' result for the coverage's transcripts; a model
    the device refuses is an SfgpuError naming the lowest offending transcript.  Usually made by CoverageDevice.project.
    result   the projection's dict (hits.GENOME_COVERAGE_STATS, state_bytes, project_ms)
    runs() -> (chrom int32, start int32, end int32, sum int64) device tensors (the bits of the unsigned values)
    write(path_or_file, chrom_names, compress=False, chunk_bytes=0)   the bedGraph file, one row per run, named by chromosome;
        compress=True: BGZF; -> the write's result dict
    close() frees the device arrays; usable as a context manager."""

    def __init__(self, coverage, placement, _event_cap=0):
        self._L = _lib.lib()
        self.device, self.M = coverage.device, coverage.M
        dev = lambda a, dt, bits: torch.from_numpy(np.ascontiguousarray(a, dt).view(bits).copy()).to(self.device)      # noqa: E731
        model = (dev(placement.status, np.uint8, np.uint8), dev(placement.chrom, np.int32, np.int32), dev(placement.strand, np.int8, np.int8),
                 dev(placement.exon_off, np.uint64, np.int64), dev(placement.exon_start, np.uint32, np.int32), dev(placement.exon_len, np.uint32, np.int32))
        if model[0].numel() != self.M or model[1].numel() != self.M or model[2].numel() != self.M or model[3].numel() != self.M + 1:
            raise ValueError(f"the placement is not one of {self.M} transcripts")
        E = int(placement.exon_off[-1])
        if model[4].numel() != E or model[5].numel() != E:
            raise ValueError(f"the placement's offsets end at {E} but it holds {model[4].numel()} block starts and {model[5].numel()} lengths")
        self.n_chrom = int(placement.n_chrom)
        self._h = None
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()
            _lib.check(self._L.sfgpu_covg_open(C.byref(h), *(_lib.ptr(t) if t.numel() else None for t in model[:3]), _lib.ptr(model[3]),
                                               *(_lib.ptr(t) if t.numel() else None for t in model[4:]), self.M, self.n_chrom, _lib.current_stream_ptr()))
        self._h = h
        if _event_cap:
            _lib.check(self._L.sfgpu_covg_event_cap(self._h, int(_event_cap)))
        self.result = None
        self.project(coverage)

    def project(self, coverage):
        """the projection of `coverage` (finished, of as many transcripts); a refusal leaves the last result in place"""
        if self._h is None or coverage._h is None:
            raise ValueError("the coverage is closed")
        res = _lib.CovgResult()
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()
            _lib.check(self._L.sfgpu_covg_project(self._h, coverage._h, C.byref(res), _lib.current_stream_ptr()))
        d = res.as_dict()
        self.result = {k: d[k] for k in d if k not in ("n_bytes", "n_chunks", "max_row_bytes", "format_ms", "d2h_ms", "sink_ms")}
        return self.result

    def runs(self):
        if self._h is None:
            raise ValueError("the genome coverage is closed")
        n = self.result["n_runs"]
        chrom, start, end = (torch.zeros(n, dtype=torch.int32, device=self.device) for _ in range(3))
        total = torch.zeros(n, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.sfgpu_covg_runs(self._h, *(_lib.ptr(t) if n else None for t in (chrom, start, end, total))))
        return chrom, start, end, total

    def write(self, path_or_file, chrom_names, compress=False, chunk_bytes=0):
        if self._h is None:
            raise ValueError("the genome coverage is closed")
        blob, off = _device_names(chrom_names, self.device)
        if off.numel() != self.n_chrom + 1:
            raise ValueError(f"{off.numel() - 1} names for {self.n_chrom} chromosomes")
        args = (self._h, _lib.ptr(blob) if blob.numel() else None, _lib.ptr(off), int(chunk_bytes))
        return _write_rows(path_or_file, self.device, compress, chunk_bytes, _lib.CovgResult(),
                           lambda sink, res: self._L.sfgpu_covg_write_text(*args, sink, None, C.byref(res), _lib.current_stream_ptr()),
                           lambda z, res: self._L.sfgpu_covg_write_bgzf(*args, z, C.byref(res), _lib.current_stream_ptr()))

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            with torch.cuda.device(self.device):
                self._L.sfgpu_covg_close(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001
            pass
