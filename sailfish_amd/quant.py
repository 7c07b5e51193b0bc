"""`sailfish quant` after the mapper -- host mirror of the driver in src/SailfishQuantify.cpp:1160-1440
(salmonQuantify) and of quasiMapReads' bookkeeping (:840-1046), over the pieces of this package.

The mapper (RapMap) is outside the path: it is replaced by whoever produces the hit records (sfgpu_hit, one per
quasi-mapping).  From there on everything the reference does is done here, in its order, on the device:

    cmd_info.json -> option checks -> per batch: hit filtering (+ bias / GC samples) -> addGroup
    -> finish -> effective lengths -> [dumpEq] -> optimize (with the bias recompute) -> quant.sf, aux/ meta
    -> [Gibbs | bootstrap samples] -> [gene-level estimates]

Return value as the reference's `int salmonQuantify`: 0 on success, 1 where it logs an error and returns 1."""
import json
import os
import time

import numpy as np
import torch

from . import efflen as _efflen
from . import genes as _genes
from . import hits as _hits
from . import writer as _writer
from .experiment import ReadExperiment, SailfishOpts, Transcripts
from .gibbs import CollapsedGibbsSampler
from .optimizer import CollapsedEMOptimizer


def write_cmd_info(out_dir, options):
    """cmd_info.json (:1262-1276): sf_version first, then the options in the order they were given."""
    os.makedirs(out_dir, exist_ok=True)
    info = [("sf_version", _writer.SAILFISH_VERSION)] + [(k, v) for k, v in (options or {}).items()]
    with open(os.path.join(out_dir, "cmd_info.json"), "w") as f:
        f.write(json.dumps(dict(info), indent=4))


def quantify(names, ref_len, hit_batches, lib_format, out_dir, sopt: SailfishOpts = None, *, seq=None, seq_off=None,
             allow_orphans=False, ignore_lib_compat=False, enforce_lib_compat=False, allow_dovetail=False,
             num_bias_samples=1_000_000, gene_map=None, cmd_options=None, seed=None, device="cuda", paired_library=None,
             detect_votes=50_000, detect_min_votes=200, detect_min_fraction=0.7, detect_max_reads=16_000_000, lib_format_counts=None):
    """names / ref_len: the index's transcripts.  hit_batches: iterable of (hits, hit_offsets) as hits.filter_hits takes
    them.  seq / seq_off: RapMapSAIndex::seq and txpOffsets (needed with biasCorrect / gcBiasCorrect).
    lib_format="A" detects the format from the records: paired_library (required then, else ValueError before anything
    is written) says which kinds vote; the incoming batches are held and their votes counted on the device (hits.library_kinds) until
    detect_votes voters are in (a convention; anything at or above detect_min_votes works), detect_max_reads reads have been seen or
    the input ends; hits.decide_library_format(votes, paired_library, detect_min_fraction, detect_min_votes) names the format, IU / U
    standing in (with a level-1 warning) where it is undetermined; the held batches and then the rest run through the loop below
    with that format, as if it had been given.  exp.lib_format_detected is then a dict: name, detected, fallback, votes, detail.
    aux/lib_format_counts.json (writer.lib_format_counts_text) is written iff lib_format is "A" or lib_format_counts is true (also with
    an explicit format): every batch is then tallied against the run's format as well.  Without either, no new call runs.
    Returns (rc, ReadExperiment)."""
    sopt = sopt or SailfishOpts()
    log = sopt.jointLog or (lambda lvl, msg: None)
    dev = torch.device(device)
    detect = isinstance(lib_format, str) and lib_format.upper() == "A"
    if detect:
        if paired_library is None:
            raise ValueError('lib_format="A" needs paired_library: whether the reads are pairs decides which records vote')
        _hits._libdet_permille(detect_min_fraction)
        if int(detect_votes) < int(detect_min_votes):
            raise ValueError(f"detect_votes = {detect_votes!r} lies below detect_min_votes = {detect_min_votes!r}: no format could ever be decided")
    start_time = time.asctime()
    write_cmd_info(out_dir, cmd_options)
    fmt = None if detect else _hits.LIBRARY_FORMATS[lib_format.upper()] if isinstance(lib_format, str) else tuple(lib_format)
    paired = bool(paired_library) if detect else fmt[0] == 1
    if sopt.numGibbsSamples > 0 and sopt.numBootstraps > 0:                  # :1280-1286
        log(2, "You cannot perform both Gibbs sampling and bootstrapping. Please choose one.")
        return 1, None
    if sopt.biasCorrect and sopt.gcBiasCorrect:                              # :1293-1297
        log(2, "Enabling both sequence-specific and fragment GC bias correction simultaneously is not yet supported. "
               "Please disable one of these options.")
        return 1, None
    if sopt.gcBiasCorrect and not paired:                                    # :1298-1309
        log(1, "Fragment GC bias correction is currently only implemented for paired-end libraries. It is being disabled")
        sopt.gcBiasCorrect = False

    exp = ReadExperiment(Transcripts(list(names), ref_len, device=dev), sopt)
    do_bias = sopt.biasCorrect or sopt.gcBiasCorrect
    gc_table = None
    if do_bias:
        if seq is None:
            raise ValueError("bias correction needs the transcript sequences (seq, seq_off)")
        exp.setSequences(seq, seq_off)
        if sopt.gcBiasCorrect:
            gc_table = _hits.gc_prefix(exp._seq, exp._seq_off, exp.transcripts().RefLength)
    eq = exp.equivalenceClassBuilder()
    eq.start()                                                               # :1319
    fl = torch.zeros(sopt.maxFragLen, dtype=torch.int32, device=dev)
    rem_fl = int(sopt.numFragSamples)                                        # remainingFLOps (:874)
    rem_bias = int(num_bias_samples)
    d_rb = torch.from_numpy(exp.readBias().view(np.int32).copy()).to(dev) if sopt.biasCorrect else None
    d_gc = torch.from_numpy(exp.observedGC().view(np.int32).copy()).to(dev) if sopt.gcBiasCorrect else None
    stats = None
    detection = counts = None
    tally_kw = dict(paired_library=paired, max_read_occs=sopt.maxReadOccs, allow_dovetail=allow_dovetail, device=dev)
    if detect:
        hit_batches, detection = _detect_library_format(hit_batches, log, detect_votes, detect_min_votes, detect_min_fraction, detect_max_reads, tally_kw)
        lib_format = detection["name"]
        fmt = _hits.LIBRARY_FORMATS[lib_format]
    for hits, off in hit_batches:                                            # the mapping threads' loop bodies
        if detect or lib_format_counts:
            _, counts = _hits.library_kinds(hits, off, expected=fmt, stats=counts, **tally_kw)
        ids, out_off, rem_fl, stats = _hits.filter_hits(hits, off, fmt, paired_library=paired, allow_orphans=allow_orphans,
                                                        ignore_lib_compat=ignore_lib_compat, enforce_lib_compat=enforce_lib_compat,
                                                        allow_dovetail=allow_dovetail, max_read_occs=sopt.maxReadOccs,
                                                        max_frag_len=sopt.maxFragLen, fl_counts=fl, remaining_fl_ops=rem_fl,
                                                        stats=stats, device=dev)
        if do_bias:
            rem_bias, _, _ = _hits.sample_bias(hits, off, fmt, exp._seq, exp._seq_off, exp.transcripts().RefLength, read_bias=d_rb,
                                               remaining_bias_samples=rem_bias, observed_gc=d_gc, gc_prefix_table=gc_table,
                                               gc_size_samp=sopt.gcSampFactor, paired_library=paired, allow_orphans=allow_orphans,
                                               max_read_occs=sopt.maxReadOccs, max_frag_len=sopt.maxFragLen, device=dev)
        eq.add_batch(ids, out_off)
    eq.finish()                                                              # :1324
    stats = stats or dict(n_observed=0, n_mapped=0, n_fwd=0, n_rc=0)
    exp.setNumObservedFragments(stats["n_observed"]); exp.setNumMappedFragments(stats["n_mapped"])
    exp.addNumFwd(stats["n_fwd"]); exp.addNumRC(stats["n_rc"])
    if d_rb is not None:
        exp.readBias()[:] = d_rb.cpu().numpy().view(np.uint32)
    if d_gc is not None:
        exp.observedGC()[:] = d_gc.cpu().numpy().view(np.uint32)
    if detect:
        exp.lib_format_detected = detection
    if detect or lib_format_counts:
        counts = counts or _hits._libdet_stats()
        name = lib_format.upper() if isinstance(lib_format, str) else _hits._FORMAT_NAMES[fmt]
        _writer.write_lib_format_counts(out_dir, sopt, _writer.lib_format_counts_text(
            name, counts, votes=detection["stats"] if detect else None, detected=detection["detected"] if detect else None,
            fallback=bool(detect and detection["fallback"])))
        exp.lib_format_counts = counts
        log(0, "library format {}: {} of {} mapped fragments have a compatible mapping (ratio {:g})".format(
            name, counts["reads_compatible"], counts["reads_mapped"], counts["reads_compatible"] / counts["reads_mapped"] if counts["reads_mapped"] else 0.0))
    # quasiMapReads' tail: the fragment length distribution and the effective lengths (:937-991, :1035-1043), then the rest
    return _quantify_tail(exp, sopt, out_dir, start_time, fl_counts=fl.cpu().numpy().view(np.uint32) if paired else None,
                          remaining_fl_ops=rem_fl, gene_map=gene_map, seed=seed)


def _owned(t):
    """a batch tensor that keeps nothing alive but itself: a view of a larger allocation (the mapper's records are the front of a
    buffer sized by a guess) is copied"""
    if isinstance(t, torch.Tensor) and t.untyped_storage().nbytes() > t.numel() * t.element_size():
        return t.clone()
    return t


def _detect_library_format(hit_batches, log, detect_votes, detect_min_votes, detect_min_fraction, detect_max_reads, tally_kw):
    """lib_format="A": batches are taken off `hit_batches` and held while their votes are counted, until detect_votes voters are in,
    detect_max_reads reads have been seen or the input ends.  -> (the batches to run: the held ones, released one by one, then the
    rest; the detection: name, detected, fallback, votes, detail, stats)"""
    it = iter(hit_batches)
    held, stats, remaining, seen = [], None, int(detect_votes), 0
    for hits, off in it:
        hits, off = _owned(hits), _owned(off)
        remaining, stats = _hits.library_kinds(hits, off, remaining_votes=remaining, stats=stats, **tally_kw)
        held.append((hits, off))
        seen += len(off) - 1
        if remaining == 0 or seen >= int(detect_max_reads):
            break
    stats = stats or _hits._libdet_stats()
    paired = tally_kw["paired_library"]
    detected, detail = _hits.decide_library_format(stats["votes_kind"], paired, detect_min_fraction, detect_min_votes)
    name = detected or ("IU" if paired else "U")
    votes = {k: v for k, v in zip(_hits.LIBDET_KINDS, stats["votes_kind"]) if v}
    if detected is None:
        log(1, "lib_format A: the library format is undetermined ({} votes in {} reads, {} needed: {}); falling back to {}: {}".format(
            detail["votes"], seen, detail["min_votes"], votes, name, _hits.format_str(_hits.LIBRARY_FORMATS[name])))
    else:
        log(0, "lib_format A: detected {} from {} votes in {} reads ({}): {}".format(name, detail["votes"], seen, votes, _hits.format_str(_hits.LIBRARY_FORMATS[name])))

    def batches():
        held.reverse()
        while held:
            yield held.pop()
        yield from it
    return batches(), dict(name=name, detected=detected, fallback=detected is None, votes=votes, detail=detail, stats=stats)


def quantify_sam(sam_path, lib_format, out_dir, sopt: SailfishOpts = None, *, transcripts_path=None, device="cuda", block_bytes=32 << 20,
                 inflate="auto", collate=False, paired=None, **kw):
    """`sailfish quant` from a mapper's SAM file on (RapMap's `quasimap -o`, bowtie2, bwa against the transcriptome; plain, BGZF or
    gzip; grouped by read name): the names and lengths come from the @SQ lines, the alignment lines are turned into hit records
    on the device (samfile.SamFile) and handed to quantify batch by batch.  `sam_path` may as well be the BAM file that
    `samtools view -b` made of that output (name-grouped, not position-sorted): the names and lengths then come from its binary
    reference list, and its record stream is parsed on the device behind the BGZF inflate.  transcripts_path: the transcript FASTA, required with
    biasCorrect / gcBiasCorrect (read with readfile.read_transcripts; its names and lengths must equal the header's, in order).
    collate: False, True or "auto", handed to samfile.SamFile: True reads a file whose lines stand in any order (a position-sorted
    SAM or BAM file, what `samtools sort` leaves) by collecting it on the device, grouping the lines by QNAME exactly and pairing
    them through their mate fields; "auto" does so iff the header says SO:coordinate.  The fragments then arrive in the order of
    their first lines, and the fragment-length sample (numFragSamples) is taken from the fragments that appear first, as always: in
    a position-sorted file those are the fragments of the first transcripts, not a sample of the whole library.
    paired: whether the file holds pairs; None takes it from the library format, and lib_format="A" (quantify's detection) requires
    it (ValueError otherwise): it is what the SamFile is opened with.
    -> (rc, experiment)"""
    from . import samfile
    sopt = sopt or SailfishOpts()
    if isinstance(lib_format, str) and lib_format.upper() == "A":
        if paired is None:
            raise ValueError('lib_format="A" needs paired=: whether the file holds pairs is what it is opened with')
        kw["paired_library"] = bool(paired)
    else:
        fmt = _hits.LIBRARY_FORMATS[lib_format.upper()] if isinstance(lib_format, str) else tuple(lib_format)
        if paired is not None and bool(paired) != (fmt[0] == 1):
            raise ValueError(f"paired = {paired!r} contradicts the library format {lib_format!r}")
        paired = fmt[0] == 1
    names, lengths = samfile.read_header(sam_path)
    if not names:
        raise ValueError(f"{sam_path}: no @SQ lines in the header")
    seq_kw = {}
    if sopt.biasCorrect or sopt.gcBiasCorrect:
        if transcripts_path is None:
            raise ValueError("bias correction needs the transcript sequences (transcripts_path)")
        from .mapper import _dollar_separated
        from .readfile import read_transcripts
        t_names, (bases, off) = read_transcripts(transcripts_path, device, inflate=inflate)
        if t_names != names or np.diff(off.cpu().numpy()).tolist() != lengths:
            raise ValueError(f"{transcripts_path}: the names and lengths of the transcripts are not those of the @SQ lines of {sam_path}")
        s, o = _dollar_separated(bases, off)
        seq_kw = dict(seq=s, seq_off=o)
    batches = samfile.SamFile(sam_path, device, bool(paired), names=names, block_bytes=block_bytes, inflate=inflate, collate=collate)
    try:
        return quantify(names, np.array(lengths, np.uint32), batches, lib_format, out_dir, sopt, device=device, **seq_kw, **kw)
    finally:
        batches.close()


def _quantify_tail(exp, sopt, out_dir, start_time, *, fl_counts, remaining_fl_ops, gene_map, seed, timings=None):
    """Everything after the class table is finished (shared by quantify and quantify_eq_classes): effective lengths
    (fl_counts None: the Gaussian prior, as a single-end run), [dumpEq], optimize with the bias recompute, quant.sf and aux/,
    [Gibbs | bootstrap samples], [gene-level estimates].  `timings`, when a dict, receives the seconds of each phase."""
    log = sopt.jointLog or (lambda lvl, msg: None)
    clock = time.perf_counter
    t0 = clock()
    if fl_counts is not None:
        _efflen.set_effective_lengths(exp, sopt, fl_counts=fl_counts, remaining_fl_ops=remaining_fl_ops)
    else:
        _efflen.set_effective_lengths(exp, sopt)
    if sopt.dumpEq:                                                          # :1331-1333
        _writer.write_equiv_counts(out_dir, exp, sopt)
    t1 = clock()
    opt = CollapsedEMOptimizer()
    log(0, "Starting optimizer:\n")
    if not opt.optimize(exp, sopt, 0.01, 10000):                             # :1343-1350
        log(2, "Encountered error during optimization.\nThis should not happen.\nPlease file a bug report on GitHub.\n")
        return 1, exp
    log(0, "Finished optimizer")
    exp.last_optimizer_stats = opt.last_stats
    t2 = clock()
    columns = _writer.abundance_columns(exp, sopt)
    if gene_map is not None:                                                 # the gene step runs after the samplers: keep what was written
        columns = columns[:2] + tuple(c.clone() for c in columns[2:])
    _writer.write_abundances(out_dir, exp, sopt, columns=columns)            # :1375
    _writer.write_meta(out_dir, exp, sopt, start_time)                       # :1377
    t3 = clock()
    if sopt.numGibbsSamples > 0:                                             # :1379-1397
        # the draws stay on the device (no per-sample callback) and are compressed there: writer.BootstrapWriter.write_device
        w = _writer.BootstrapWriter(out_dir, sopt)
        gs = CollapsedGibbsSampler()
        ok = gs.sample(exp, sopt, None, sopt.numGibbsSamples, seed=seed)
        try:
            if ok:
                w.write_device(gs.last_samples)
        finally:
            w.close()
        if not ok:
            return 1, exp
    elif sopt.numBootstraps > 0:                                             # :1398-1413
        w = _writer.BootstrapWriter(out_dir, sopt)
        ok = opt.gatherBootstraps(exp, sopt, None, 0.01, 10000, seed=seed)
        try:
            if ok:
                w.write_device(opt.last_bootstraps)
        finally:
            w.close()
        if not ok:
            return 1, exp
    t4 = clock()
    if gene_map is not None:                                                 # :1416-1426
        try:
            # from the columns just written, on the device: quant.sf is not read back (genes.aggregate_columns).  Only what the
            # reference catches here (std::invalid_argument: an unreadable map, :1419) is logged and passed over; a failure of the
            # device path (_lib.SfgpuError, or a TypeError for columns that are not device tensors) is no map error and is raised,
            # as every other device failure of this function is: there is no quiet fall-back to the host loop
            # (the names go as the device pair quant.sf was written from: the join with the map happens on the device too)
            _genes.generate_gene_level_estimates(gene_map, out_dir, agg_key=sopt.txpAggregationKey,
                                                 columns=(exp.transcripts().name_blob(),) + tuple(columns[1:]))
        except ValueError as e:
            log(2, f"Error: [{e}] when trying to compute gene-level estimates. The gene-level file(s) may not exist")
    if timings is not None:
        timings.update(efflen_s=t1 - t0, optimize_s=t2 - t1, write_s=t3 - t2, samples_s=t4 - t3, genes_s=clock() - t4)
    return 0, exp


def quantify_eq_classes(names, ref_len, eq_paths, out_dir, sopt: SailfishOpts = None, *, fld_counts=None, num_mapped=None,
                        num_observed=None, observed_bias=None, observed_gc=None, num_fwd=None, num_rc=None, seq=None, seq_off=None,
                        gene_map=None, cmd_options=None, seed=None, device="cuda"):
    """Quantify from saved class tables (--readEqClasses, src/SailfishQuantify.cpp:1114 and loadEquivClasses :1444-1494,
    both commented out in the reference): the classes of every file in `eq_paths` (eq_classes.txt as write_equiv_counts
    writes it; several files -- lanes, runs -- fold into one table, equal labels adding their counts) are parsed on the device,
    then the same tail as quantify() runs: effective lengths, [dumpEq], optimize, quant.sf, aux/, [bootstrap | Gibbs], [genes].

    names / ref_len: the transcripts; every file must list exactly these names in this order.
    fld_counts: the fragment-length counts of the run (maxFragLen entries); None selects the Gaussian prior, as a single-end run.
    num_mapped / num_observed: default to the sum of the class counts (the loader's accounting).
    observed_bias (4096) / observed_gc (101) and num_fwd / num_rc: what biasCorrect / gcBiasCorrect read; the class files do
    not hold them, so they are required with those options (an all-ones vector is the untouched pseudo-count, never collected).
    Returns (rc, ReadExperiment) like quantify(); exp.timings holds the seconds of each phase."""
    sopt = sopt or SailfishOpts()
    log = sopt.jointLog or (lambda lvl, msg: None)
    dev = torch.device(device)
    clock = time.perf_counter
    t0 = clock()
    if sopt.numGibbsSamples > 0 and sopt.numBootstraps > 0:                  # :1280-1286
        log(2, "You cannot perform both Gibbs sampling and bootstrapping. Please choose one.")
        return 1, None
    if sopt.biasCorrect and sopt.gcBiasCorrect:                              # :1293-1297
        log(2, "Enabling both sequence-specific and fragment GC bias correction simultaneously is not yet supported. "
               "Please disable one of these options.")
        return 1, None
    for on, vec, n, what in ((sopt.biasCorrect, observed_bias, 4096, "observed_bias (biasCorrect)"),
                             (sopt.gcBiasCorrect, observed_gc, 101, "observed_gc (gcBiasCorrect)")):
        if not on:
            continue
        if vec is None:
            raise ValueError(f"{what} is required: the class files do not hold the observed bias counts")
        vec = np.asarray(vec)
        if vec.shape != (n,):
            raise ValueError(f"{what} must hold {n} counts, got shape {vec.shape}")
        if np.all(vec == 1):
            raise ValueError(f"{what} is all ones, the pseudo-count a run starts from: it was never collected "
                             "(the original run did not use this bias correction)")
    do_bias = sopt.biasCorrect or sopt.gcBiasCorrect
    if do_bias:
        if seq is None:
            raise ValueError("bias correction needs the transcript sequences (seq, seq_off)")
        if num_fwd is None or num_rc is None:
            raise ValueError("bias correction needs num_fwd / num_rc, the strand split of the mapped fragments")
    start_time = time.asctime()
    write_cmd_info(out_dir, cmd_options)
    exp = ReadExperiment(Transcripts(list(names), ref_len, device=dev), sopt)
    if do_bias:
        exp.setSequences(seq, seq_off)
        if sopt.biasCorrect:
            exp.readBias()[:] = np.asarray(observed_bias).astype(np.uint32)
        if sopt.gcBiasCorrect:
            exp.observedGC()[:] = np.asarray(observed_gc).astype(np.uint32)
        exp.addNumFwd(num_fwd); exp.addNumRC(num_rc)
    eq = exp.equivalenceClassBuilder()
    eq.start()
    t1 = clock()
    from . import eqfile as _eqfile
    _, exp.eqfile_results = _eqfile.fold_files(eq, eq_paths, names=exp.transcripts().RefName)
    eq.finish()
    t2 = clock()
    exp.setNumMappedFragments(eq.total_reads if num_mapped is None else num_mapped)
    exp.setNumObservedFragments(eq.total_reads if num_observed is None else num_observed)
    exp.timings = dict(setup_s=t1 - t0, load_s=t2 - t1)
    return _quantify_tail(exp, sopt, out_dir, start_time, fl_counts=fld_counts, remaining_fl_ops=0, gene_map=gene_map, seed=seed,
                          timings=exp.timings)


def fld_counts_for_requant(stored, sopt: SailfishOpts):
    """The FLD argument of quantify_eq_classes that reproduces a finished run's effective lengths from its aux/fld.gz (the
    stored counts themselves, writer.write_meta): counts equal, element for element, to efflen.normal_counts(sopt) mean the
    run took the Gaussian-prior branch (single end, or too few unique pairs) -> None; any other counts are the empirical
    distribution the run used -> those counts."""
    stored = np.asarray(stored, dtype=np.int32)
    prior = _efflen.normal_counts(sopt)
    if stored.shape == prior.shape and np.array_equal(stored, prior):
        return None
    return stored.astype(np.uint32)


def read_run(prev_dir, sopt: SailfishOpts = None):
    """The inputs of a finished run, from its output directory: names and integer Length (quant.sf), the class file
    (aux/eq_classes.txt), the stored FLD counts (aux/fld.gz), num_mapped / num_processed (aux/meta_info.json) and the observed
    bias vectors (aux/observed_bias.gz, aux/observed_gc.gz)."""
    import gzip
    sopt = sopt or SailfishOpts()
    aux = os.path.join(prev_dir, sopt.auxDir)
    names, lengths = [], []
    with open(os.path.join(prev_dir, "quant.sf")) as f:
        head = f.readline().rstrip("\n").split("\t")
        if head[:3] != ["Name", "Length", "EffectiveLength"]:
            raise ValueError(f"{os.path.join(prev_dir, 'quant.sf')}: not a quant.sf header: {head}")
        for line in f:
            row = line.rstrip("\n").split("\t")
            names.append(row[0]); lengths.append(int(row[1]))
    with open(os.path.join(aux, "meta_info.json")) as f:
        meta = json.load(f)

    def vec(name, dt):
        with gzip.open(os.path.join(aux, name), "rb") as g:
            return np.frombuffer(g.read(), dtype=dt).copy()
    return dict(names=names, ref_len=np.asarray(lengths, np.uint32), eq_path=os.path.join(aux, "eq_classes.txt"),
                fld=vec("fld.gz", np.int32), num_mapped=int(meta["num_mapped"]), num_processed=int(meta["num_processed"]),
                observed_bias=vec("observed_bias.gz", np.int32), observed_gc=vec("observed_gc.gz", np.int32))


def requantify(prev_dir, out_dir, sopt: SailfishOpts = None, *, seq=None, seq_off=None, num_fwd=None, num_rc=None, gene_map=None,
               cmd_options=None, seed=None, device="cuda"):
    """Quantify again from a finished run's output directory (written with dumpEq), without mapping: switch EM <-> VBEM, add
    bootstraps or Gibbs draws, add a gene map.  Inputs come from read_run(prev_dir).  Effective lengths are recomputed (quant.sf
    prints them with %g), and the FLD branch is the original run's: stored counts equal to efflen.normal_counts(sopt) element for
    element -> the Gaussian prior, else the stored counts (fld_counts_for_requant).  sopt must carry the original maxFragLen
    and prior mean / SD.  With biasCorrect / gcBiasCorrect the sequences and the strand split num_fwd / num_rc (not part of a
    run's output) are required as well."""
    sopt = sopt or SailfishOpts()
    run = read_run(prev_dir, sopt)
    return quantify_eq_classes(run["names"], run["ref_len"], [run["eq_path"]], out_dir, sopt,
                               fld_counts=fld_counts_for_requant(run["fld"], sopt), num_mapped=run["num_mapped"],
                               num_observed=run["num_processed"],
                               observed_bias=run["observed_bias"] if sopt.biasCorrect else None,
                               observed_gc=run["observed_gc"] if sopt.gcBiasCorrect else None, num_fwd=num_fwd, num_rc=num_rc,
                               seq=seq, seq_off=seq_off, gene_map=gene_map, cmd_options=cmd_options, seed=seed, device=device)
