"""Quasi-mapping front end on the device -- where the reference calls RapMap (SACollector inside processReadsQuasi,
src/SailfishQuantify.cpp:141-142, 192-213, 487-488, 526-528): reads in, the hit records of sailfish_amd.hits out.

RapMap is not part of the reference tree (fetched at build time); this is an exact-seed mapper with its own contract
(csrc/mapper.hip), not RapMap's suffix-array search, and parity with RapMap is unpinned.  Host side: sequence packing
(bytes + offsets), batching, and the driver `quantify_reads` = index -> map -> quantify()."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .hits import HIT_DTYPE, _call_with_room


def pack_sequences(seqs, device="cpu"):
    """list of str / bytes -> (uint8 tensor of the bases back to back, int64 offsets[n + 1])"""
    raw = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    off = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    buf = np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8).copy()
    return torch.from_numpy(buf).to(device), torch.from_numpy(off).to(device)


class QuasiIndex:
    """k-mer index of a transcriptome on the device (sfgpu_index_build)."""

    def __init__(self, sequences, k=31, max_occ=1000, device="cuda", seeds=2, seed_len=None):
        """seed_len: None = the library's default (scan mode, seeds of min(19, k) bases, matches extended to maximal length);
        0 = the end-seed contract (`seeds` exact k-mers per strand); 8 .. k = scan mode with seeds of that length.
        sequences: a list of str / bytes, or a (uint8 tensor, int64 offsets) pair already packed (readfile.read_transcripts)"""
        self.device = torch.device(device)
        self._L = _lib.lib()
        if isinstance(sequences, tuple):
            seq, off = (t.to(self.device) for t in sequences)
        else:
            seq, off = pack_sequences(sequences, self.device)
        self.ref_len = (off[1:] - off[:-1]).to(torch.int32).contiguous()
        self.M = int(off.numel()) - 1
        self._keep = (seq.contiguous(), off[:-1].contiguous())
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()
            _lib.check(self._L.sfgpu_index_build(C.byref(self._h), _lib.ptr(self._keep[0]), _lib.ptr(self._keep[1]), _lib.ptr(self.ref_len),
                                                 self.M, int(k), int(max_occ), _lib.current_stream_ptr()))
        kk, npos, nk = C.c_uint32(), C.c_uint64(), C.c_uint64()
        _lib.check(self._L.sfgpu_index_info(self._h, C.byref(kk), C.byref(npos), C.byref(nk)))
        self.k, self.n_positions, self.n_kmers = kk.value, npos.value, nk.value
        self.seeds = 2
        self.seed_len = min(19, self.k)
        if seed_len is not None:
            self.set_scan(seed_len)
        if seeds != 2:
            self.set_seeds(seeds)
            if seed_len is None:
                self.set_scan(0)                           # asking for S end seeds selects the end-seed contract

    def set_scan(self, seed_len):
        """sfgpu_index_set_scan: 0 = end seeds; 8 .. k = scan mode (maximal-match extension) with seeds of that length"""
        _lib.check(self._L.sfgpu_index_set_scan(self._h, int(seed_len)))
        self.seed_len = int(seed_len)

    def set_seeds(self, seeds):
        """seeds per strand (sfgpu_index_set_seeds): 2 = offsets 0 and len - k, every hit kept; 3 .. 8 = seeds spread evenly over
        the read, only the (transcript, strand) pairs that the most seeds hit are kept (more sensitive on reads with errors)"""
        _lib.check(self._L.sfgpu_index_set_seeds(self._h, int(seeds)))
        self.seeds = int(seeds)

    def map_reads(self, reads1, reads2=None, validate=None, tags=False, rescue=None):
        """reads1 / reads2: lists of str / bytes, or (uint8 tensor, int64 offsets) pairs already packed.
        rescue: None, or a dict of hits.rescue_mates' keywords (min_identity, window; {} = its defaults) for a paired batch (else
        ValueError): before anything is validated, the reads that have nothing but orphan records have their orphans' transcripts
        searched for the missing mate, and where one is placed the read's records become pairs; `last_rescue_stats` holds the pass's
        counters and `last_rescue_mism` the placed mates' mismatches, one '<u2' per record handed to the validation.
        validate: None, or a dict of hits.verify_hits' keywords (min_identity, keep_best, max_indel; {} = its defaults): the records are then
        verified against the transcripts' bases before they are returned, and `last_scores` / `last_verify_stats` hold the
        survivors' scores and the pass's counters.  With "align": True beside a max_indel of 1 .. 15 (else ValueError) the survivors
        are then aligned with gaps (hits.align_hits): `last_alignments` holds (pos, nm, op_off, ops), two slots per surviving record,
        as SamDeviceWriter.write(alignments=) takes them, and `last_align_stats` the pass's counters.
        "tags": True in `validate`, or tags=True where nothing is validated: the NM / MD tags of the records that are returned
        (hits.md_tags, over `last_alignments` where there are any) are left as `last_tags` = (nm, md_off, md), as
        SamDeviceWriter.write(tags=) takes them, with the pass's counters as `last_tag_stats`; both are None otherwise.
        -> (hits: uint8 device tensor [n_hits * 24] of HIT_DTYPE records, offsets: int32 device tensor [R + 1])"""
        align = False
        if validate is not None and "tags" in validate:
            validate = dict(validate)
            tags = bool(validate.pop("tags")) or bool(tags)
        if validate is not None and "align" in validate:
            validate = dict(validate)
            align = bool(validate.pop("align"))
            if align and not 1 <= int(validate.get("max_indel", 0)) <= 15:
                raise ValueError('validate: "align" needs a max_indel of 1 .. 15')
        dev = self.device
        s1, o1 = reads1 if isinstance(reads1, tuple) else pack_sequences(reads1)
        s1, o1 = s1.to(dev).contiguous(), o1.to(dev).contiguous()
        n = int(o1.numel()) - 1
        s2 = o2 = None
        if reads2 is not None:
            s2, o2 = reads2 if isinstance(reads2, tuple) else pack_sequences(reads2)
            s2, o2 = s2.to(dev).contiguous(), o2.to(dev).contiguous()
            assert int(o2.numel()) - 1 == n, "both mate files hold the same number of reads"
        off = torch.empty(n + 1, dtype=torch.int32, device=dev)
        n_hits = C.c_uint64(0)

        def call(hits, cap):
            rc = self._L.sfgpu_map_reads(self._h, _lib.ptr(s1), _lib.ptr(o1), _lib.ptr(s2), _lib.ptr(o2), n, _lib.ptr(hits), cap, _lib.ptr(off),
                                         C.byref(n_hits), _lib.current_stream_ptr())
            return rc, n_hits.value
        with torch.cuda.device(dev):
            torch.cuda.current_stream().synchronize()            # (a second call only if the first capacity guess was too small)
            hits, n_rec = _call_with_room(max(4 * n, 1024), lambda cap: torch.empty(cap * 24, dtype=torch.uint8, device=dev), call)
        hits = hits[: n_rec * 24]
        if rescue is not None:
            from .hits import rescue_mates
            hits, off, self.last_rescue_mism, self.last_rescue_stats = rescue_mates(self, hits, off, (s1, o1), None if s2 is None else (s2, o2), **rescue)
        if validate is not None:
            from .hits import verify_hits
            hits, off, self.last_scores, self.last_verify_stats = verify_hits(self, hits, off, (s1, o1), None if s2 is None else (s2, o2), **validate)
            self.last_alignments = self.last_align_stats = None
            if align:
                from .hits import align_hits
                *aln, self.last_align_stats = align_hits(self, hits, off, (s1, o1), None if s2 is None else (s2, o2), max_indel=validate["max_indel"])
                self.last_alignments = tuple(aln)
        self.last_tags = self.last_tag_stats = None
        if tags:
            from .hits import md_tags
            *t, self.last_tag_stats = md_tags(self, hits, off, (s1, o1), None if s2 is None else (s2, o2),
                                              alignments=self.last_alignments if validate is not None else None)
            self.last_tags = tuple(t)
        return hits, off

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.sfgpu_index_destroy(self._h); self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def hits_to_numpy(hits, offsets):
    return hits.cpu().numpy().view(HIT_DTYPE), offsets.cpu().numpy().view(np.uint32)


def _validation(validate_mappings, min_identity, keep_best, max_indel=0):
    """-> (the `validate` dict for QuasiIndex.map_reads or None, the counters to accumulate over the batches); ValueError at once
    for a min_identity outside 0 .. 1 or a max_indel outside 0 .. 15, before anything is indexed"""
    if not validate_mappings:
        return None, None
    from .hits import VERIFY_STATS, VERIFYG_STATS, _max_indel, _permille
    _permille(min_identity)
    k = _max_indel(max_indel)
    if not k:
        return dict(min_identity=min_identity, keep_best=bool(keep_best)), dict.fromkeys(VERIFY_STATS, 0)
    return dict(min_identity=min_identity, keep_best=bool(keep_best), max_indel=k), dict.fromkeys(VERIFYG_STATS, 0)


def _rescue(rescue_mates, rescue_window, min_identity, paired, lib_format, sopt):
    """-> (the `rescue` dict for QuasiIndex.map_reads or None, the counters to accumulate over the batches); ValueError at once for
    a single-end run, a library format whose mates do not face each other, a min_identity outside 0 .. 1 or a window outside
    1 .. 2^20 (None: sopt.maxFragLen), before anything is indexed"""
    if not rescue_mates:
        return None, None
    from .experiment import SailfishOpts
    from .hits import LIBRARY_FORMATS, RESCUE_STATS, TOWARD, _permille, _rescue_window
    if not paired:
        raise ValueError("rescue_mates=True needs a paired run: a single-end read has no mate to rescue")
    fmt = LIBRARY_FORMATS.get(lib_format.upper()) if isinstance(lib_format, str) else None if lib_format is None else tuple(lib_format)
    if fmt is None or fmt[0] != 1 or fmt[1] != TOWARD:
        raise ValueError(f"rescue_mates=True searches for inward-facing mates: the library format {lib_format!r} is not one of IU, ISF, ISR")
    _permille(min_identity)
    window = _rescue_window((sopt if sopt is not None else SailfishOpts()).maxFragLen if rescue_window is None else rescue_window)
    return dict(min_identity=min_identity, window=window), dict.fromkeys(RESCUE_STATS, 0)


# the passes of a batch whose counters a run adds up: (name, QuasiIndex's attribute after map_reads, the keys that are maxima, not sums)
_PASSES = (("rescue", "last_rescue_stats", ()), ("verify", "last_verify_stats", ()), ("align", "last_align_stats", ("scratch_bytes",)), ("tag", "last_tag_stats", ("max_md_bytes",)))


def _is_sink(x):
    return isinstance(x, (str, bytes, os.PathLike)) or hasattr(x, "write")


class _UnmappedWriters:
    """The ReadDeviceWriters behind write_unmapped=, one per mate file.  write() takes a batch as it is handed to quant.quantify: a
    read goes out iff the batch holds no record for it (offsets[r + 1] == offsets[r]); the selector is computed on the device, and
    both mates go out with the same one, so the files stay in step."""

    @staticmethod
    def targets(write_unmapped, unmapped_compress, paired):
        """write_unmapped= of quantify_reads / quantify_files: ValueError unless it is one path or binary file object for a
        single-end run and a pair of them for a paired one.  -> the targets as a tuple, or None"""
        if write_unmapped is None:
            if unmapped_compress:
                raise ValueError("unmapped_compress=True needs write_unmapped")
            return None
        if not paired:
            if not _is_sink(write_unmapped):
                raise ValueError("write_unmapped: one path or binary file object for a single-end run")
            return (write_unmapped,)
        if not (isinstance(write_unmapped, (tuple, list)) and len(write_unmapped) == 2 and all(_is_sink(x) for x in write_unmapped)):
            raise ValueError("write_unmapped: a pair of paths or binary file objects for a paired run, one for either mate file")
        return tuple(write_unmapped)

    def __init__(self, targets, compress):
        from .readfile import ReadDeviceWriter
        self.writers = []
        self.reads = self.unmapped = 0
        try:
            for t in targets:
                self.writers.append(ReadDeviceWriter(t, compress=compress))
        except BaseException:
            self.close()
            raise

    def write(self, offsets, mates, quals, names):
        """mates / quals / names: one entry per writer -- (bases, offsets), the qualities or None, the name pair or None"""
        select = offsets[1:] == offsets[:-1]
        for w, reads, q, nm in zip(self.writers, mates, quals, names):
            written = w.write(reads, quals=q, names=nm, select=select)
        self.reads += int(offsets.numel()) - 1
        self.unmapped += written

    def close(self):
        for w in self.writers:
            w.close()

    def stats(self):
        return dict(reads=self.reads, unmapped=self.unmapped, bytes=[w.stats["bytes"] for w in self.writers])


def _host_names(names):
    """the transcripts' names as a host list; names on the device give their bytes, never decoded"""
    if isinstance(names, tuple) and isinstance(names[0], torch.Tensor):
        blob, off = (x.cpu().numpy() for x in names)
        return [blob[a:b].tobytes() for a, b in zip(off[:-1].tolist(), off[1:].tolist())]
    return names


class _MappingsRun:
    """What quantify_reads and quantify_files share from the mapper's call to the files beside the estimates: the
    options' checks, the two kinds of writers, a batch's map -> rescue -> validate -> align -> tag -> write, the counters added up over the
    batches, and their report.  Constructed before anything is indexed: it raises the options' ValueErrors."""

    def __init__(self, paired, write_mappings, mappings_format, mappings_oriented, mappings_sorted, validate_mappings, min_identity, keep_best, max_indel,
                 mappings_gapped, mappings_tags, write_unmapped, unmapped_compress, rescue_mates=False, rescue_window=None, lib_format=None, sopt=None,
                 mappings_posteriors=False, write_coverage=None, coverage_weights="posterior", coverage_compress=False, out_dir=None,
                 write_genome_coverage=None, coverage_annotation=None, write_genome_mappings=None, genome_annotation=None, genome_sizes=None):
        from .hits import ALIGNG_STATS, MDTAG_STATS, POSTERIOR_STATS
        if write_genome_mappings is None and (genome_annotation is not None or genome_sizes is not None):
            raise ValueError("genome_annotation and genome_sizes need write_genome_mappings")
        if write_genome_mappings is not None:
            if not _is_sink(write_genome_mappings):
                raise ValueError("write_genome_mappings: one path or binary file object")
            if genome_annotation is None and coverage_annotation is None:
                raise ValueError("write_genome_mappings needs genome_annotation (the GTF with the exons), or coverage_annotation to serve as it")
            if genome_annotation is not None and coverage_annotation is not None and os.fspath(genome_annotation) != os.fspath(coverage_annotation):
                raise ValueError(f"one run reads one annotation: genome_annotation is {genome_annotation!r}, coverage_annotation {coverage_annotation!r}")
            if genome_annotation is None:
                genome_annotation = coverage_annotation
        any_mappings = write_mappings is not None or write_genome_mappings is not None
        if coverage_weights not in ("posterior", "uniform"):
            raise ValueError(f'coverage_weights is "posterior" or "uniform", not {coverage_weights!r}')
        if write_coverage is None and write_genome_coverage is None and coverage_compress:
            raise ValueError("coverage_compress=True needs write_coverage or write_genome_coverage")
        if write_coverage is not None and not _is_sink(write_coverage):
            raise ValueError("write_coverage: one path or binary file object")
        if (write_genome_coverage is None) != (coverage_annotation is None) and not (write_genome_coverage is None and write_genome_mappings is not None):
            raise ValueError("write_genome_coverage and coverage_annotation (the GTF with the exons) come together")
        if write_genome_coverage is not None and not _is_sink(write_genome_coverage):
            raise ValueError("write_genome_coverage: one path or binary file object")
        if mappings_sorted and mappings_format != "bam":
            raise ValueError(f'mappings_sorted=True needs mappings_format="bam", not {mappings_format!r}')
        self.rescue, rstats = _rescue(rescue_mates, rescue_window, min_identity, paired, lib_format, sopt)
        self.validate, vstats = _validation(validate_mappings, min_identity, keep_best, max_indel)
        astats = tstats = None
        if mappings_gapped:
            if not any_mappings or not validate_mappings or not (self.validate or {}).get("max_indel"):
                raise ValueError("mappings_gapped=True needs write_mappings or write_genome_mappings, validate_mappings=True and a max_indel of 1 .. 15")
            self.validate, astats = dict(self.validate, align=True), dict.fromkeys(ALIGNG_STATS, 0)
        if mappings_tags:
            if not any_mappings or not mappings_oriented:
                raise ValueError("mappings_tags=True needs write_mappings or write_genome_mappings, and mappings_oriented=True")
            tstats = dict.fromkeys(MDTAG_STATS, 0)
        if mappings_posteriors and not any_mappings:
            raise ValueError("mappings_posteriors=True needs write_mappings or write_genome_mappings")
        # With posteriors the reads pass twice: the first pass decides the records and quantifies them without a mappings
        # file, the second maps them again and writes the file with the estimates' weights.  `second`: which pass batch() serves;
        # `again`: the second pass's rescue / verify counters, which must reproduce the first's.
        self.posteriors, self.second, self.weights, self.again = bool(mappings_posteriors), False, None, None
        # The coverage file is that of the records the mappings file shows.  With posterior weights it is accumulated in
        # the second pass, which then runs for it alone too (opening no mappings file); with uniform weights in the first.
        # The genome file is the same coverage projected through the annotation's exons, so either file opens the
        # CoverageDevice; the annotation is read here, before anything is indexed: a bad line fails early.
        self.cov_sink, self.cov_compress, self.cov_dir = write_coverage, bool(coverage_compress), out_dir
        self.covg_sink, self.covg_model, self.covg_stats = write_genome_coverage, None, None
        # The genome mappings file is the mappings file's batch projected through the same kind of model and written by a
        # second SamDeviceWriter over the chromosomes; where both genome files are asked for, the GTF is read once.
        self.gsink, self.gmodel, self.gsizes, self.galn, self.gsam, self.galn_stats = write_genome_mappings, None, None, None, None, None
        if write_genome_coverage is not None or write_genome_mappings is not None:
            from .genes import ExonModel
            model = ExonModel.from_gtf(coverage_annotation if write_genome_coverage is not None else genome_annotation)
            self.covg_model = model if write_genome_coverage is not None else None
            if write_genome_mappings is not None:
                self.gmodel, self.gsizes = model, model.chrom_lengths(genome_sizes)
        self.cov_wanted = write_coverage is not None or write_genome_coverage is not None
        self.cov_posterior = self.cov_wanted and coverage_weights == "posterior"
        self.gapped = bool(mappings_gapped)
        self.two_pass = self.posteriors or self.cov_posterior
        self.cov = self.cov_stats = None
        self.stats = dict(rescue=rstats, verify=vstats, align=astats, tag=tstats)  # None: the pass does not run
        self.post_stats = dict.fromkeys(POSTERIOR_STATS, 0) if self.posteriors else None
        self.targets, self.compress = _UnmappedWriters.targets(write_unmapped, unmapped_compress, paired), unmapped_compress
        self.paired, self.sink = paired, write_mappings
        self.sam_kw = dict(format=mappings_format, oriented=mappings_oriented, sort="coordinate" if mappings_sorted else None)
        self.mapped, self.unmapped = any_mappings, self.targets is not None       # which files the run writes
        self.sam = self.unm = None

    def open(self, names, idx):
        """the SamDeviceWriter behind write_mappings= and the ReadDeviceWriters behind write_unmapped="""
        if self.mapped and not self.posteriors:              # (with posteriors the file is opened by second_pass)
            self._open_sam(names, idx)
        if self.unmapped:
            self.unm = _UnmappedWriters(self.targets, self.compress)
        if self.cov_wanted:
            from .coverage import CoverageDevice
            self.cov = CoverageDevice(idx.ref_len, idx.device)

    def _open_sam(self, names, idx):
        from .samfile import SamDeviceWriter
        if self.sink is not None:
            self.sam = SamDeviceWriter(self.sink, names, idx.ref_len.cpu().numpy().view(np.uint32), self.paired, **self.sam_kw)
        if self.gsink is not None:
            from .hits import GENOME_ALN_STATS, GenomeAlignments
            placement = self.gmodel.for_names(_host_names(names))
            self.galn = GenomeAlignments(placement, idx.device)
            self.gsam = SamDeviceWriter(self.gsink, placement.chrom_names, self.gsizes, self.paired, **self.sam_kw)
            self.galn_stats = dict(dict.fromkeys(GENOME_ALN_STATS, 0), transcripts=len(placement.status), transcripts_placed=int((placement.status == 0).sum()))

    def batch(self, idx, r1, r2, *, quals=(None, None), sam_quals=True, read_names=None, mate_names=(None, None)):
        """One batch: mapped (validated, aligned, tagged, as the options say), its counters added, and written to the run's files.
        r1 / r2: what map_reads takes (packed pairs on the device where the run writes a file); quals / mate_names: one entry per mate
        file; sam_quals: whether the mappings file takes the qualities too; read_names: its QNAMEs.  -> (hits, offsets)"""
        opt = {} if self.rescue is None else dict(rescue=self.rescue)              # (without the option the call is the one it was)
        writing = self.sam is not None or self.gsam is not None
        sam_now = writing and self.second == self.posteriors       # the pass that writes the mappings files: the second with posteriors
        cov_now = self.cov is not None and self.second == self.cov_posterior    # ... that adds to the coverage: the second with posterior weights
        first = self.two_pass and not self.second
        validate = self.validate
        if validate is not None and not (sam_now or (cov_now and self.gapped)) and (self.two_pass or not writing):
            validate = {key: v for key, v in validate.items() if key != "align"}      # only what decides the records runs: map -> rescue -> validate
        aligned = validate is not None and bool(validate.get("align"))
        tagged = self.stats["tag"] is not None and (sam_now or not self.two_pass)
        h, o = idx.map_reads(r1, r2, validate=validate, tags=tagged, **opt)
        for name, attr, maxima in _PASSES:
            total = self.stats[name]
            if total is None or (name == "align" and not (aligned and (sam_now or not self.two_pass))) or (name == "tag" and not tagged):
                continue
            if self.second and name in ("rescue", "verify"):
                total = self.again[name]
            for key, v in getattr(idx, attr).items():
                total[key] = max(total[key], v) if key in maxima else total[key] + v
        post = {}
        if self.second:
            from .hits import posteriors
            *values, st = posteriors(h, o, self.weights)
            post = dict(posteriors=tuple(values)) if self.posteriors else {}
            for key, v in st.items() if self.post_stats is not None else ():
                self.post_stats[key] = max(self.post_stats[key], v) if key == "max_records" else self.post_stats[key] + v
        if cov_now:
            aln = None
            if aligned:
                a_pos, _, a_off, a_ops = idx.last_alignments[:4]
                aln = (a_pos, a_off, a_ops)
            self.cov.add(h, o, posteriors=values[0] if self.cov_posterior else None, alignments=aln)
        if sam_now:
            q1, q2 = quals if sam_quals else (None, None)
            reads = dict(read_names=read_names, seqs=r1 if r2 is None else (r1, r2), quals=None if q1 is None and q2 is None else q1 if r2 is None else (q1, q2))
            aln, tags = idx.last_alignments if self.stats["align"] is not None else None, idx.last_tags if self.stats["tag"] is not None else None
            if self.sam is not None:
                self.sam.write(h, o, **reads, alignments=aln, tags=tags, **post)
            if self.gsam is not None:                     # the same batch in genome terms: projected, its per-record values gathered, written
                from .hits import GENOME_ALN_STATS, project_alignments
                g_h, g_o, g_aln, g_tags, src, st = project_alignments(h, o, self.galn, aln, tags)
                for key in GENOME_ALN_STATS:
                    self.galn_stats[key] += st[key]
                g_post = dict(posteriors=tuple(v[src.long()] for v in post["posteriors"])) if post else {}
                self.gsam.write(g_h, g_o, **reads, alignments=g_aln, tags=g_tags, **g_post)
        if self.unm is not None and not self.second:
            self.unm.write(o, (r1,) if r2 is None else (r1, r2), quals, mate_names)
        return h, o

    def second_pass(self, rc, exp, sopt, names, idx, batches):
        """mappings_posteriors=True, behind quant.quantify: where that returned 0, the weights NumReads / EffectiveLength of the final
        estimates (full doubles on the device; 0 where EffectiveLength <= 0 or the quotient is not finite; left on the experiment as
        `posterior_weights`), the mappings file opened, and batches() -- the reads, produced again -- run through batch() once more.
        RuntimeError where the second pass's rescue or verify counters are not the first's: the file would not show the records that
        were quantified."""
        if not self.two_pass:
            return
        log = (getattr(sopt, "jointLog", None) if sopt is not None else None) or (lambda lvl, msg: None)
        if rc != 0 or exp is None:
            self.post_stats = None
            if self.posteriors:
                log(1, "mappings_posteriors: the quantification did not succeed (rc {}), so no mappings file is written".format(rc))
            if self.cov_posterior and self.cov_sink is not None:
                log(1, "write_coverage: the quantification did not succeed (rc {}), so no coverage file is written".format(rc))
            if self.cov_posterior and self.covg_sink is not None:
                log(1, "write_genome_coverage: the quantification did not succeed (rc {}), so no genome coverage file is written".format(rc))
            return
        from . import writer
        _, _, length, _, est = writer.abundance_columns(exp, sopt)
        w = est.to(torch.float64) / length.to(torch.float64)
        self.weights = exp.posterior_weights = torch.where((length > 0) & torch.isfinite(w), w, torch.zeros_like(w)).contiguous()
        self.second = True
        self.again = {name: dict.fromkeys(self.stats[name], 0) for name in ("rescue", "verify") if self.stats[name] is not None}
        if self.posteriors:
            self._open_sam(names, idx)
        for _ in batches():
            pass
        for name, again in self.again.items():
            if again != self.stats[name]:
                raise RuntimeError(f"mappings_posteriors: the second pass over the reads gave other {name} counters ({again}) than the first "
                                   f"({self.stats[name]}): the mappings file does not show the records that were quantified")

    def write_coverage(self, names, sopt):
        """write_coverage= and write_genome_coverage=, behind the last pass: the runs found and the rows formatted on the device
        (coverage.CoverageDevice), the transcript file (only with write_coverage) and aux/coverage_summary.tsv written; then the runs
        projected onto the chromosomes (coverage.GenomeCoverageDevice) and the genome file written.  With posterior weights and a
        quantification that failed there is no second pass and nothing is written."""
        if self.cov is None or (self.cov_posterior and not self.second):
            return
        res = self.cov.finish()
        wrote = self.cov.write(self.cov_sink, names, compress=self.cov_compress) if self.cov_sink is not None else dict(n_bytes=0)
        if self.covg_sink is not None:
            placement = self.covg_model.for_names(_host_names(names))
            with self.cov.project(placement) as g:
                gw = g.write(self.covg_sink, placement.chrom_names, compress=self.cov_compress)
                self.covg_stats = dict(g.result, transcripts=self.cov.M, bytes=int(gw["n_bytes"]))
        if self.cov_dir is not None:
            aux = os.path.join(self.cov_dir, getattr(sopt, "auxDir", "aux") if sopt is not None else "aux")
            os.makedirs(aux, exist_ok=True)
            self.cov.write_summary(os.path.join(aux, "coverage_summary.tsv"), names)
        self.cov_stats = dict(self.cov.stats, runs=res["runs"], bases_covered=res["bases_covered"], bases_total=res["bases_total"], residue=res["residue"],
                              state_bytes=res["state_bytes"], bytes=int(wrote["n_bytes"]), weights="posterior" if self.cov_posterior else "uniform")

    def close(self):
        for w in (self.sam, self.gsam, self.galn, self.unm, self.cov):
            if w is not None:
                w.close()

    def report(self, exp, sopt):
        """every pass's counters on the experiment (`rescue_stats`, `verify_stats`, `align_stats`, `tag_stats`: None where the pass did not run;
        `unmapped_stats` only with write_unmapped) and one line each to sopt.jointLog"""
        res, v, a, t = (self.stats[name] for name, _, _ in _PASSES)
        u = None if self.unm is None else self.unm.stats()
        ps = self.post_stats if self.second else None
        if exp is not None:
            exp.rescue_stats, exp.verify_stats, exp.align_stats, exp.tag_stats = res, v, a, t
            exp.posterior_stats = ps
            exp.coverage_stats = self.cov_stats
            exp.genome_coverage_stats = self.covg_stats
            exp.genome_mappings_stats = self.galn_stats
            if u is not None:
                exp.unmapped_stats = u
        log = getattr(sopt, "jointLog", None) if sopt is not None else None
        if log is None:
            return
        if res is not None:
            log(0, "rescued mates (min identity {:g}, window {}): {} reads had orphan records only ({} records); {} of them now pair, with {} records; "
                   "{} of their orphans found no mate and were dropped; {} mismatches in the placed mates".format(
                       self.rescue["min_identity"], self.rescue["window"], res["reads_eligible"], res["records_orphan"], res["reads_rescued"],
                       res["records_rescued"], res["records_dropped"], res["sum_mism"]))
        val = self.validate
        if v is not None and val.get("max_indel"):
            log(0, "validated mappings (min identity {:g}, max indel {}{}): {} of {} records kept ({} below the identity, {} not the best of their read); "
                   "{} of {} mapped reads keep a record; {} edits in the kept records; {} records kept only with gaps".format(
                       val["min_identity"], val["max_indel"], ", best only" if val["keep_best"] else "", v["records_out"], v["records_in"],
                       v["failed_identity"], v["dropped_not_best"], v["reads_out"], v["reads_in"], v["sum_edits"], v["rescued"]))
        elif v is not None:
            log(0, "validated mappings (min identity {:g}{}): {} of {} records kept ({} below the identity, {} not the best of their read); "
                   "{} of {} mapped reads keep a record; {} mismatches in the kept records".format(
                       val["min_identity"], ", best only" if val["keep_best"] else "", v["records_out"], v["records_in"],
                       v["failed_identity"], v["dropped_not_best"], v["reads_out"], v["reads_in"], v["sum_mism"]))
        if a is not None:
            log(0, "gapped mappings: {} of {} mates traced through the band; {} mismatches, inserted and deleted bases in the written alignments; "
                   "{} mates unalignable".format(a["jobs_traced"], a["jobs"], a["sum_nm"], a["unalignable"]))
        if t is not None:
            log(0, "tagged mappings: NM, MD and NH on {} lines, {} of them <len>M without a mismatch; NM sums to {}; {} MD bytes, the longest MD {}".format(
                t["slots"], t["slots_plain"], t["sum_nm"], t["md_bytes"], t["max_md_bytes"]))
        if ps is not None:
            log(0, "posteriors in the mappings file: ZW on the {} records of {} mapped reads, {} of them with more than one record (the largest has {}); "
                   "{} reads have no weight at all and are spread evenly; {} records are written as 0".format(
                       ps["records"], ps["reads_mapped"], ps["reads_multi"], ps["max_records"], ps["reads_flat"], ps["records_zero"]))
        if self.cov_stats is not None:
            c = self.cov_stats
            log(0, "coverage ({} weights): {} lines, {} empty intervals; {} runs over {} of {} bases; the device held {} bytes".format(
                c["weights"], c["lines"], c["empty_intervals"], c["runs"], c["bases_covered"], c["bases_total"], c["state_bytes"]))
        if self.covg_stats is not None:
            c = self.covg_stats
            log(0, "genome coverage: {} of {} transcripts placed; {} pieces, {} events; {} runs over {} bases; {} bases dropped as unplaced, {} off the "
                   "model; the device held {} bytes".format(c["transcripts_placed"], c["transcripts"], c["n_pieces"], c["n_events"], c["n_runs"],
                                                            c["bases_covered"], c["bases_unplaced"], c["bases_off_model"], c["state_bytes"]))
            if c["transcripts_placed"] == 0:
                log(1, "write_genome_coverage: the annotation places none of the {} transcripts (the names are matched byte for byte)".format(c["transcripts"]))
            if c["transcripts_length_mismatch"] > 0:
                log(1, "write_genome_coverage: the exons of {} placed transcripts do not sum to the transcript's length; bases beyond the exons "
                       "are dropped".format(c["transcripts_length_mismatch"]))
        if self.galn_stats is not None:
            c = self.galn_stats
            log(0, "genome mappings: {} of {} transcripts placed; {} of {} records written ({} on transcripts that are not placed, {} unalignable, {} off "
                   "the chromosome's range); {} reads lost every record; {} lines, {} of them spliced by {} N operations, {} reversed; {} columns beyond "
                   "the exons; {} words in, {} out".format(c["transcripts_placed"], c["transcripts"], c["records_out"], c["records_in"], c["records_unplaced"],
                                                           c["records_unalignable"], c["records_off_range"], c["reads_emptied"], c["lines"], c["lines_spliced"],
                                                           c["n_operations"], c["lines_reversed"], c["columns_beyond_model"], c["words_in"], c["words_out"]))
            if c["transcripts_placed"] == 0:
                log(1, "write_genome_mappings: the annotation places none of the {} transcripts (the names are matched byte for byte)".format(c["transcripts"]))
        if u is not None:
            log(0, "unmapped reads: {} of {} reads have no record and were written, {} bytes of {}".format(
                u["unmapped"], u["reads"], " + ".join(str(b) for b in u["bytes"]), "FASTQ" if self.unm.writers[0].format == 2 else "FASTA"))


def quantify_reads(names, sequences, reads1, reads2, lib_format, out_dir, sopt=None, *, k=31, batch_reads=1_000_000, device="cuda",
                   write_mappings=None, mappings_format="sam", quals1=None, quals2=None, mappings_oriented=False, mappings_sorted=False,
                   validate_mappings=False, min_identity=0.9, keep_best=False, max_indel=0, mappings_gapped=False, mappings_tags=False,
                   write_unmapped=None, unmapped_compress=False, rescue_mates=False, rescue_window=None, mappings_posteriors=False,
                   write_coverage=None, coverage_weights="posterior", coverage_compress=False, write_genome_coverage=None, coverage_annotation=None,
                   write_genome_mappings=None, genome_annotation=None, genome_sizes=None, **kw):
    """`sailfish quant` from the reads on: index the transcriptome, map the reads in batches (the reference's parser jobs),
    and hand the hit records to quant.quantify (filtering, classes, effective lengths, EM, writers).  write_mappings: a path (or a
    binary file object) that receives every mapped batch as SAM, formatted on the device (samfile.SamDeviceWriter) before the batch
    is quantified: QNAME r<index of the read>, SEQ the read's bases; the estimates do not depend on it.  mappings_format is
    SamDeviceWriter's `format` ("sam"; "sam.gz" for the text, "bam" for BAM records, in BGZF members encoded on the device); it is never
    inferred from the path.  quals1 / quals2: the reads' qualities (lists like reads1 / reads2, of as many bytes a read as it has
    bases), written as QUAL; default '*'.  mappings_oriented=True puts the lines with 0x10 on the transcript's strand, as the SAM
    specification stores them (SEQ reverse-complemented, QUAL reversed): the file other tools expect.  mappings_sorted=True (with
    mappings_format="bam", else ValueError) writes the file coordinate-sorted with its .bai index beside it (SamDeviceWriter's
    sort="coordinate": the records stay on the device until the run ends); the estimates never depend on it.
    validate_mappings=True verifies every batch's records against the transcripts' bases (hits.verify_hits with min_identity and
    keep_best) before the batch is written and quantified: the mappings file and the estimates see the same, surviving records; the
    counters of all batches are left on the experiment as `verify_stats` and go to sopt.jointLog as one line.  max_indel = 1 .. 15
    (with validate_mappings; outside 0 .. 15: ValueError) scores every mate with gaps -- its banded edit distance within max_indel
    diagonals of the recorded one -- so reads that carry an indel keep their true records; `verify_stats` then holds `sum_edits` for
    `sum_mism`, and `rescued`: the records kept only with gaps.  The mappings file receives the surviving records as before: its
    CIGAR and POS still describe the recorded diagonal, not the gapped alignment -- unless mappings_gapped=True (it needs write_mappings,
    validate_mappings=True and max_indel >= 1, else ValueError before anything is indexed): then every surviving mate is aligned
    through the band on the device (hits.align_hits) and its line carries that alignment's POS and CIGAR (I, D and soft clips where the
    mate hangs over an end), PNEXT following; with every mappings_format, mappings_oriented and mappings_sorted.  The estimates never
    depend on it; the counters are left on the experiment as `align_stats` and go to sopt.jointLog as one line.  (A surviving mate
    with no base on its transcript -- possible only at a min_identity near 0 -- fails the batch, as it does without the option.)
    mappings_tags=True (it needs write_mappings and mappings_oriented=True, else ValueError before anything is indexed: NM and MD
    describe the read on the transcript's strand) ends every mapped line with NM:i: (the line's edit distance), MD:Z: (its mismatch
    string) and NH:i: (the read's record count), computed on the device after validation and alignment for the surviving records
    (hits.md_tags), with every mappings_format, with mappings_sorted, and with and without mappings_gapped and validate_mappings.  The
    estimates never depend on it; the counters are left on the experiment as `tag_stats` and go to sopt.jointLog as one line.
    write_unmapped: where the reads that did not map go, as a read file formatted on the device (readfile.ReadDeviceWriter): one path
    or binary file object for a single-end run, a pair of them (mate 1, mate 2) for a paired one, anything else a ValueError before
    anything is indexed.  A read is written iff the batch handed to quant.quantify holds no record for it -- after validation,
    keep_best and the gapped pass; a pair with one orphan record is mapped; what the hit filter decides later does not enter --
    which are the reads of the 4 / 77 / 141 lines of the mappings file.  Both mates go out with the same selector.  The records are
    called r<index of the read>, FASTQ where quals1 (quals2) is given, else FASTA.  unmapped_compress=True (it needs write_unmapped)
    writes BGZF files.  Neither the estimates nor the mappings file depend on it; the counts are left on the experiment as
    `unmapped_stats` (reads, unmapped, bytes per file) and go to sopt.jointLog as one line.
    rescue_mates=True (a paired run with an inward-facing library format -- IU, ISF, ISR -- else ValueError before anything is
    indexed) searches, in every batch and before any validation, for the missing mates of the reads that mapped as orphans only
    (hits.rescue_mates): each orphan's transcript, on the opposite strand, ungapped, inside the window a fragment of at most
    rescue_window bases allows (None: sopt.maxFragLen; outside 1 .. 2^20: ValueError); a mate is placed where at least min_identity
    of its bases match (the same keyword as the validation's, whether or not validate_mappings is on), and the read's records then
    are pairs like any the mapper made: validation, alignment, tags, the mappings and unmapped files and the estimates see them so.
    The search stays ungapped with max_indel > 0; the validation then scores the rescued pair with gaps like every record.  The
    counters are left on the experiment as `rescue_stats` (None without the option) and go to sopt.jointLog as one line.
    mappings_posteriors=True (it needs write_mappings, else ValueError before anything is indexed) ends every mapped line of the
    mappings file with ZW:f:<p>, RSEM's tag: the posterior probability, under the run's final estimates, that the read came from that
    record -- the record's weight NumReads / EffectiveLength over the sum of the weights of the read's records ("%g"; hits.posteriors;
    both lines of a pair carry their record's value).  The estimates exist only after the EM, so the reads pass twice: the first pass
    maps, rescues and validates the batches and quantifies them as ever, but opens no mappings file; the second, run iff the
    quantification returned 0 (else no mappings file is created, and the log says so), slices the reads again, maps them again and
    writes the file, with every mappings_format, mappings_oriented, mappings_sorted, mappings_gapped, mappings_tags, validate_mappings
    and rescue_mates setting.  quant.sf, aux/ and the unmapped files are byte for byte those of the run without the option, and so
    is the mappings file but for the tag.  ZW is a posterior over the records the file shows: what the hit filter drops later
    (library compatibility, orphans, maxReadOccs) does not enter -- the same sentence write_unmapped carries.  The rescue and verify
    counters reported are the first pass's, and the second must reproduce them (RuntimeError otherwise); the align and tag counters
    are the second's; the pass's own are left on the experiment as `posterior_stats` (None without the option), its weights as
    `posterior_weights`, and go to sopt.jointLog as one line.
    lib_format="A" detects the library format from the first batches' records (quant.quantify: the detect_* keywords and
    lib_format_counts pass through **kw; whether mate 2 exists says which records vote) and writes aux/lib_format_counts.json; with
    rescue_mates=True it is a ValueError before anything is indexed: the rescue needs to know that the pairs face inward.
    write_coverage: a path (or a binary file object) that receives the coverage of the transcripts as bedGraph -- name, start, end,
    depth, 0-based and half open, a row per maximal stretch of equal nonzero depth, no header line -- accumulated, scanned and
    formatted on the device (coverage.CoverageDevice); aux/coverage_summary.tsv gets every transcript's covered fraction, mean and
    largest depth.  It is the coverage of the mappings file the same options would write: the records after rescue and validation,
    the gapped alignment's intervals iff mappings_gapped=True, else the recorded diagonal, a pair's two lines counted each.
    coverage_weights="posterior" (the default) weighs a record by the posterior probability the ZW tag is made from, so the reads
    pass twice as with mappings_posteriors -- also without write_mappings, no mappings file being opened then -- and a run whose
    quantification failed writes no coverage file and says so in the log; "uniform" gives each of a read's n records 1 / n and
    accumulates in the first pass; anything else is a ValueError before anything is indexed, as is coverage_compress=True (a BGZF
    file, encoded on the device) without a coverage file.  The estimates never depend on it; the counters are left on the experiment
    as `coverage_stats` (None without the option) and go to sopt.jointLog as one line.
    write_genome_coverage: a path (or a binary file object) that receives the same coverage in GENOME coordinates -- chromosome, start,
    end, depth, the rows of write_coverage's shape, sorted by the chromosomes' names bytewise and then by start, which is what
    bedGraphToBigWig and the genome browsers take -- with coverage_annotation, the GTF (plain or gzip) whose `exon` records place the
    transcripts: genes.ExonModel reads it on the host before anything is indexed, matches transcript_id to the transcripts' names byte
    for byte, and the device projects every run through the exon blocks, adds the isoforms' contributions per genomic base and
    formats the rows (coverage.GenomeCoverageDevice, csrc/covgfmt.h).  Either keyword without the other, or a value that is neither a
    path nor a binary file object, is a ValueError before anything is indexed.  It works with or without write_coverage (the
    transcript file is written only with that; aux/coverage_summary.tsv in both cases); coverage_weights and coverage_compress govern
    both files, and with posterior weights a failed quantification writes neither and the log says so for each.  Transcripts the
    annotation does not place (genes.EXON_STATUS) and bases beyond a transcript's exons are dropped and counted; the counters are left
    on the experiment as `genome_coverage_stats` (None without the option) and go to sopt.jointLog as one line, with a warning where
    no transcript is placed or where exons do not sum to a transcript's length.
    write_genome_mappings: a path (or a binary file object) that receives the mappings in GENOME coordinates -- what `rsem
    --output-genome-bam` is for: RNAME a chromosome, POS on it, introns as N in the CIGAR, reverse-strand transcripts turned round
    (FLAG 0x10 / 0x20, SEQ, QUAL, the CIGAR's order and the MD all follow) -- with genome_annotation, the GTF whose `exon` records place
    the transcripts (read once, on the host, before anything is indexed; where only coverage_annotation is given it serves; two
    different annotations in one run are a ValueError), and optionally genome_sizes, a chrom.sizes / .fai-style file for the @SQ
    lengths (genes.ExonModel.chrom_lengths: without it LN is the furthest exon end, a lower bound).  Every batch of the mappings
    file is projected on the device (hits.project_alignments, csrc/galnfmt.h) behind map, rescue, validate, align, tag and the
    posteriors, and written by a second SamDeviceWriter over the chromosomes: the file obeys mappings_format, mappings_oriented,
    mappings_sorted (with its .bai), mappings_gapped, mappings_tags and mappings_posteriors as the transcript file does, and is
    written in the same pass.  write_mappings is not required: the options that need a mappings file take either.  Records on
    transcripts the annotation does not place, lines without a reference column and lines that leave [0, 2^31 - 1] are dropped and
    counted; a read that keeps none is written unmapped; NH is the number of records the genome file shows for the read, and ZW
    the transcript file's value, gathered and not renormalised over the kept records.  The estimates, the
    transcript file and every other output never depend on it; the counters are left on the experiment as `genome_mappings_stats`
    (None without the option) and go to sopt.jointLog as one line, with a warning where no transcript is placed.
    -> (rc, experiment)"""
    from . import quant
    run = _MappingsRun(reads2 is not None, write_mappings, mappings_format, mappings_oriented, mappings_sorted, validate_mappings, min_identity, keep_best, max_indel,
                       mappings_gapped, mappings_tags, write_unmapped, unmapped_compress, rescue_mates, rescue_window, lib_format, sopt, mappings_posteriors,
                       write_coverage, coverage_weights, coverage_compress, out_dir, write_genome_coverage, coverage_annotation, write_genome_mappings,
                       genome_annotation, genome_sizes)
    if run.two_pass and sopt is None:                      # (the second pass reads the columns under the options the run had)
        from .experiment import SailfishOpts
        sopt = SailfishOpts()
    idx = QuasiIndex(sequences, k=k, device=device)
    n = len(reads1)

    def batches():
        for a in range(0, n, batch_reads):
            b = min(n, a + batch_reads)
            r1, r2 = reads1[a:b], None if reads2 is None else reads2[a:b]
            q1 = q2 = None
            if run.mapped or run.unmapped:                   # the bases are wanted on the device beyond the mapper's call
                r1 = tuple(t.to(idx.device) for t in pack_sequences(r1))
                r2 = None if r2 is None else tuple(t.to(idx.device) for t in pack_sequences(r2))
                q1 = None if quals1 is None else pack_sequences(quals1[a:b])[0].to(idx.device)
                q2 = None if quals2 is None or r2 is None else pack_sequences(quals2[a:b])[0].to(idx.device)
            yield run.batch(idx, r1, r2, quals=(q1, q2))
    seq_kw = {}
    if sopt is not None and (getattr(sopt, "biasCorrect", False) or getattr(sopt, "gcBiasCorrect", False)):
        s, o = pack_sequences([x + "$" if isinstance(x, str) else bytes(x) + b"$" for x in sequences])
        seq_kw = dict(seq=bytes(s.numpy().tobytes()), seq_off=o[:-1].numpy())
    try:
        run.open(names, idx)
        rc, exp = quant.quantify(names, idx.ref_len.cpu().numpy().view(np.uint32), batches(), lib_format, out_dir, sopt, device=device,
                                 paired_library=reads2 is not None, **seq_kw, **kw)
        run.second_pass(rc, exp, sopt, names, idx, batches)
        run.write_coverage(names, sopt)
    finally:
        run.close()
        idx.close()
    run.report(exp, sopt)
    return rc, exp


def _dollar_separated(bases, off):
    """packed transcripts -> (the bytes with a '$' behind every transcript, where each begins): what the bias models take"""
    b, o = bases.cpu().numpy(), off.cpu().numpy()
    M, total = len(o) - 1, int(o[-1])
    out = np.full(total + M, ord("$"), np.uint8)
    out[np.arange(total) + np.repeat(np.arange(M), np.diff(o))] = b[:total]
    return out.tobytes(), o[:-1] + np.arange(M)


def quantify_files(transcripts_path, reads1_path, reads2_path, lib_format, out_dir, sopt=None, *, k=31, batch_reads=1_000_000, device="cuda",
                   inflate="auto", write_mappings=None, mappings_format="sam", mappings_oriented=False, check_mate_names=False, mappings_sorted=False,
                   validate_mappings=False, min_identity=0.9, keep_best=False, max_indel=0, mappings_gapped=False, mappings_tags=False,
                   write_unmapped=None, unmapped_compress=False, rescue_mates=False, rescue_window=None, mappings_posteriors=False,
                   write_coverage=None, coverage_weights="posterior", coverage_compress=False, write_genome_coverage=None, coverage_annotation=None,
                   write_genome_mappings=None, genome_annotation=None, genome_sizes=None, **kw):
    """`sailfish quant` from the files on: the transcript FASTA and the read files (FASTA or FASTQ, plain or gzip; reads2_path =
    None: single end) are parsed on the device (readfile.ReadFile), the mate files in lockstep, batch_reads records each; the
    batches are mapped and handed to quant.quantify as in quantify_reads.  `inflate` is ReadFile's: where gzip files are inflated.
    write_mappings and mappings_format as in quantify_reads; QNAME is the record's name in the mate 1 file up to its first space or tab (the names
    stay on the device from the parser to the writer: ReadFile(names="device")).  check_mate_names=True compares the names of the two
    mates of every read on the device (readfile.mate_names_match: equal but for a trailing /1 or /2) and raises ValueError at the first
    read where the files are out of step, naming the record counted from the start of the files and both names
    (a single-end run, reads2_path = None, has no mates: the keyword then does nothing).  mappings_oriented=True writes the file other tools expect: the read files are
    opened with quals=True, so QUAL is the FASTQ's quality line ('*' for FASTA reads), and the lines with 0x10 carry SEQ
    reverse-complemented and QUAL reversed.  mappings_sorted, validate_mappings, min_identity, keep_best, max_indel, mappings_gapped and
    mappings_tags as in quantify_reads; so are rescue_mates and rescue_window, and mappings_posteriors: the second pass then opens the read files again, with the
    same ReadFile options.  write_unmapped and unmapped_compress as in quantify_reads: the reads without a record go out
    as they came in -- each mate file's own names up to the first space or tab (names="device" on both files), bases and quality lines
    (quals=True on both, also when mappings_oriented is off: QUAL of the mappings file is then still '*'); a FASTA read file gives a
    FASTA unmapped file.  No name, base or offset visits the host.  write_coverage, coverage_weights, coverage_compress,
    write_genome_coverage and coverage_annotation as in quantify_reads (the transcripts' names are matched to the annotation by
    their bytes as the FASTA has them).  write_genome_mappings, genome_annotation and genome_sizes as in quantify_reads.
    -> (rc, experiment)"""
    from . import quant
    from .readfile import ReadFile, mate_names_match, read_transcripts
    run = _MappingsRun(reads2_path is not None, write_mappings, mappings_format, mappings_oriented, mappings_sorted, validate_mappings, min_identity, keep_best, max_indel,
                       mappings_gapped, mappings_tags, write_unmapped, unmapped_compress, rescue_mates, rescue_window, lib_format, sopt, mappings_posteriors,
                       write_coverage, coverage_weights, coverage_compress, out_dir, write_genome_coverage, coverage_annotation, write_genome_mappings,
                       genome_annotation, genome_sizes)
    if run.two_pass and sopt is None:                      # (the second pass reads the columns under the options the run had)
        from .experiment import SailfishOpts
        sopt = SailfishOpts()
    names, (bases, off) = read_transcripts(transcripts_path, device, inflate=inflate)
    idx = QuasiIndex((bases, off), k=k, device=device)
    keep = run.mapped and bool(mappings_oriented)            # the mappings file carries QUAL

    def batches():
        check = bool(check_mate_names) and reads2_path is not None
        f1 = ReadFile(reads1_path, device, names="device" if run.mapped or check or run.unmapped else False, inflate=inflate, quals=keep or run.unmapped)
        f2 = None if reads2_path is None else ReadFile(reads2_path, device, names="device" if check or run.unmapped else False, inflate=inflate,
                                                       quals=keep or run.unmapped)
        done = 0                                              # records of the batches before this one
        try:
            while True:
                r1 = f1.read(batch_reads)
                r2 = None if f2 is None else f2.read(batch_reads)
                n = int(r1[1].numel()) - 1
                if r2 is not None and int(r2[1].numel()) - 1 != n:
                    raise ValueError(f"{reads1_path} and {reads2_path} do not hold the same number of records")
                if n == 0:
                    break
                if check:
                    bad = mate_names_match(f1.last_names, f2.last_names)
                    if bad is not None:                       # only these two names are copied back
                        nm1, nm2 = (bytes(b[int(o[bad]):int(o[bad + 1])].cpu().numpy()) for b, o in (f1.last_names, f2.last_names))
                        raise ValueError(f"{reads1_path} and {reads2_path} are out of step at record {done + bad}: "
                                         f"{nm1.decode('utf-8', 'replace')!r} against {nm2.decode('utf-8', 'replace')!r}")
                done += n
                yield run.batch(idx, r1, r2, quals=(f1.last_quals, None if f2 is None else f2.last_quals), sam_quals=keep, read_names=f1.last_names,
                                mate_names=(f1.last_names, None if f2 is None else f2.last_names))
        finally:
            f1.close()
            if f2 is not None:
                f2.close()
    seq_kw = {}
    if sopt is not None and (getattr(sopt, "biasCorrect", False) or getattr(sopt, "gcBiasCorrect", False)):
        s, o = _dollar_separated(bases, off)
        seq_kw = dict(seq=s, seq_off=o)
    try:
        run.open(names, idx)
        rc, exp = quant.quantify(names, idx.ref_len.cpu().numpy().view(np.uint32), batches(), lib_format, out_dir, sopt, device=device,
                                 paired_library=reads2_path is not None, **seq_kw, **kw)
        run.second_pass(rc, exp, sopt, names, idx, batches)
        run.write_coverage(names, sopt)
    finally:
        run.close()
        idx.close()
    run.report(exp, sopt)
    return rc, exp
