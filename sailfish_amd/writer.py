"""quant.sf / aux/ output -- host mirror of src/GZipWriter.cpp:51-92 (eq_classes.txt), :94-192 (writeMeta),
:194-248 (quant.sf) and :249-285 (writeBootstrap)."""
import gzip
import json
import os

import numpy as np
import torch

from . import _lib
from .experiment import ReadExperiment, SailfishOpts


def tpm(readExp: ReadExperiment, sopt: SailfishOpts):
    """TPM column (GZipWriter.cpp:216-245), computed on the device; returns a float64 tensor."""
    txps = readExp.transcripts()
    length = txps.ref_length_f64() if sopt.noEffectiveLengthCorrection else txps.EffectiveLength
    out = torch.zeros(len(txps), dtype=torch.float64, device=txps.device)
    with torch.cuda.device(txps.device):
        _lib.check(_lib.lib().sfgpu_tpm(_lib.ptr(txps.estCount), _lib.ptr(length.contiguous()), len(txps),
                                        float(readExp.numMappedFragments()), _lib.ptr(out), _lib.current_stream_ptr()))
    return out, length


def fmt_g(x):
    """cppformat `{}` for double == printf %g (6 significant digits), include/spdlog/details/format.h:2898-2914."""
    return "%g" % x


def abundance_columns(readExp: ReadExperiment, sopt: SailfishOpts):
    """The columns of quant.sf where they lie: (names, Length, EffectiveLength, TPM, NumReads) -- the host list of names, the
    32-bit integer device tensor of reference lengths and three float64 device tensors.  What write_abundances writes and what
    the gene-level step (genes.aggregate_columns) folds."""
    txps = readExp.transcripts()
    t, length = tpm(readExp, sopt)          # (without the length correction `length` is the reference lengths as doubles)
    return txps.RefName, txps.RefLength, length, t, txps.estCount


def write_abundances(path, readExp: ReadExperiment, sopt: SailfishOpts, columns=None):
    """writeAbundances (GZipWriter.cpp:194-248): Name, Length, EffectiveLength, TPM, NumReads.  The header line is written
    here; the rows are formatted on the device from the columns where they lie (quantfile.write_file, sfgpu_quant_write_text).
    The bytes are quantfile.format_rows', the per-row loop over fmt_g this function used to run.  `columns`: what
    abundance_columns returned for this experiment, when the caller holds it already."""
    from . import quantfile
    _, ref_len, length, t, est = columns if columns is not None else abundance_columns(readExp, sopt)
    os.makedirs(path, exist_ok=True)
    quantfile.write_file(os.path.join(path, "quant.sf"), readExp.transcripts().name_blob(), ref_len, length, t, est)
    return True


def write_equiv_counts(path, readExp: ReadExperiment, sopt: SailfishOpts):
    """writeEquivCounts (GZipWriter.cpp:51-92): aux/eq_classes.txt (canonical class order).  The header is written here; the
    class lines are formatted on the device from the builder's table (eqfile.write_file, sfgpu_eqvec_write_text)."""
    from . import eqfile
    aux = os.path.join(path, sopt.auxDir)
    os.makedirs(aux, exist_ok=True)
    eqfile.write_file(os.path.join(aux, "eq_classes.txt"), readExp.transcripts().RefName, readExp.equivalenceClassBuilder().eqVec())
    return True


SAILFISH_VERSION = "0.10.0"        # sailfish::version (include/SailfishConfig.hpp:32), the release mirrored here
NUM_BIAS_BINS = 4 ** 6             # ReadKmerDist<6>::counts (include/ReadExperiment.hpp:249, ReadKmerDist.hpp:16)


def write_meta(path, readExp: ReadExperiment, sopt: SailfishOpts, start_time: str):
    """writeMeta (GZipWriter.cpp:94-192): aux/bootstrap/names.tsv.gz when sampling is requested, aux/fld.gz and
    the bias-model vectors expected_bias.gz (float64[4096]) / observed_bias.gz (int32[4096]) / expected_gc.gz
    (float64[101]) / observed_gc.gz (int32[101]) (:145-162; all ones without bias correction, as in the reference)
    and aux/meta_info.json (cereal JSON: same keys, same order).  One difference, outside the hot path: fld.gz
    holds the stored fragment-length counts themselves (the reference writes a random_device-seeded 10 000-sample
    realisation of them, EmpiricalDistribution.cpp:125-143)."""
    txps = readExp.transcripts()
    aux = os.path.join(path, sopt.auxDir)
    os.makedirs(aux, exist_ok=True)
    n_boot = int(sopt.numBootstraps)
    n_samp = n_boot if n_boot > 0 else int(sopt.numGibbsSamples)
    if n_samp > 0:
        if len(txps) == 0:
            return False
        bs = os.path.join(aux, "bootstrap")
        os.makedirs(bs, exist_ok=True)
        with gzip.open(os.path.join(bs, "names.tsv.gz"), "wb", compresslevel=6) as f:
            f.write(("\t".join(txps.RefName) + "\n").encode())
    fld = readExp.fragLengthDist()
    fld = np.zeros(sopt.maxFragLen, np.int32) if fld is None else np.asarray(fld, np.int32)
    with gzip.open(os.path.join(aux, "fld.gz"), "wb", compresslevel=6) as f:
        f.write(fld.tobytes())                                   # writeVectorToFile: raw little-endian binary
    for name, vec, dt in (("expected_bias.gz", readExp.expectedSeqBias(), np.float64), ("observed_bias.gz", readExp.readBias(), np.int32),
                          ("expected_gc.gz", readExp.expectedGCBias(), np.float64), ("observed_gc.gz", readExp.observedGC(), np.int32)):
        with gzip.open(os.path.join(aux, name), "wb", compresslevel=6) as f:
            f.write(np.ascontiguousarray(vec).astype(dt).tobytes())
    samp_type = "bootstrap" if n_boot > 0 else ("gibbs" if n_samp > 0 else "none")
    n_obs = readExp.numObservedFragments() or readExp.numMappedFragments()
    info = [("sf_version", SAILFISH_VERSION), ("samp_type", samp_type),
            ("frag_dist_length", int(len(fld) - 1)),             # EmpiricalDistribution::maxValue() of vals = 0..n-1
            ("bias_correct", bool(sopt.biasCorrect)), ("num_bias_bins", NUM_BIAS_BINS),
            ("num_targets", len(txps)), ("num_bootstraps", n_boot),
            ("num_processed", int(n_obs)), ("num_mapped", int(readExp.numMappedFragments())),
            ("percent_mapped", (readExp.numMappedFragments() / n_obs * 100.0) if n_obs else 0.0),
            ("call", "quant"), ("start_time", start_time)]
    with open(os.path.join(aux, "meta_info.json"), "w") as f:
        f.write(json.dumps(dict(info), indent=4))
    return True


def lib_format_counts_text(expected, counts, votes=None, detected=None, fallback=False):
    """The text of aux/lib_format_counts.json, keys in a fixed order.  expected: the name of the format the run used; counts: the
    hits.library_kinds stats of all its batches, tallied with expected= that format; votes: the stats that hold the detection's votes
    (None: no detection ran, the votes are zeros); detected: the name the detection decided on, or None; fallback: the detection was
    undetermined and `expected` is the unstranded default.  compatible_fragment_ratio = num_compatible / num_mapped (0 when nothing
    mapped); strand_mapping_bias = the minority share of the two reads_kind counters of the expected orientation (ISF and ISR for an
    inward format, SF and SR for a single-end one; 0 when both are 0)."""
    from .hits import AWAY, LIBDET_KINDS, LIBRARY_FORMATS, NONE, TOWARD
    name = expected.upper()
    orientation = LIBRARY_FORMATS[name][1]
    first = {TOWARD: 0, AWAY: 2, NONE: 10}.get(orientation, 4)
    a, b = (int(counts["reads_kind"][first + i]) for i in (0, 1))
    mapped, compatible = int(counts["reads_mapped"]), int(counts["reads_compatible"])
    vk = [int(v) for v in votes["votes_kind"]] if votes is not None else [0] * len(LIBDET_KINDS)
    per_kind = lambda vals: {k: int(v) for k, v in zip(LIBDET_KINDS, vals)}
    info = [("expected_format", name), ("detected", detected), ("fallback", bool(fallback)), ("num_votes", sum(vk)), ("votes", per_kind(vk)),
            ("num_reads", int(counts["reads"])), ("num_mapped", mapped), ("num_over_occs", int(counts["reads_over_occs"])),
            ("num_consistent", mapped - int(counts["reads_mixed"])), ("num_mixed", int(counts["reads_mixed"])), ("num_compatible", compatible),
            ("compatible_fragment_ratio", compatible / mapped if mapped else 0.0),
            ("strand_mapping_bias", min(a, b) / (a + b) if a + b else 0.0),
            ("records", per_kind(counts["records_kind"])), ("reads", per_kind(counts["reads_kind"]))]
    return json.dumps(dict(info), indent=4)


def write_lib_format_counts(path, sopt: SailfishOpts, text):
    aux = os.path.join(path, sopt.auxDir)
    os.makedirs(aux, exist_ok=True)
    with open(os.path.join(aux, "lib_format_counts.json"), "w") as f:
        f.write(text)
    return True


class BootstrapWriter:
    """writeBootstrap<T> (GZipWriter.cpp:249-285): every sample is appended as raw binary (float64 for
    bootstrap replicates, int32 for Gibbs samples) to aux/bootstrap/bootstraps.gz.  An instance is the callback
    of EMProblem.bootstrap / gibbs_sample (the C ABI calls it one sample at a time, in draw order); it compresses on the host
    (zlib level 6, one sample at a time).  write_device takes the samplers' n x M device matrix instead and produces the same
    payload through the device encoder (gzfile.GzDeviceWriter).  One instance uses one of the two ways."""
    ROWS_BYTES = 256 << 20          # write_device hands the matrix over in row slices of at most this many bytes

    def __init__(self, path, sopt: SailfishOpts, logger=None):
        self._dir = os.path.join(path, sopt.auxDir, "bootstrap")
        self._f = None
        self._gz = None
        self._log = logger
        self.written = 0

    def __call__(self, abund):
        if self._gz is not None:
            raise RuntimeError("BootstrapWriter: samples were already written with write_device; one file takes one of the two ways")
        if self._f is None:
            os.makedirs(self._dir, exist_ok=True)
            self._f = gzip.open(os.path.join(self._dir, "bootstraps.gz"), "wb", compresslevel=6)
        self._f.write(np.ascontiguousarray(abund).tobytes())
        self.written += 1
        if self._log:
            self._log(0, f"wrote {self.written} bootstraps")
        return True

    def write_device(self, samples):
        """`samples`: 2-D contiguous device tensor, one sample per row in draw order (float64 replicates, int32 Gibbs draws)."""
        from . import gzfile
        if self._f is not None:
            raise RuntimeError("BootstrapWriter: samples were already written one by one; one file takes one of the two ways")
        if not (isinstance(samples, torch.Tensor) and samples.is_cuda and samples.dim() == 2 and samples.is_contiguous()):
            raise TypeError("write_device expects a contiguous 2-D device tensor, one sample per row")
        if self._gz is None:
            os.makedirs(self._dir, exist_ok=True)
            self._gz = gzfile.GzDeviceWriter(os.path.join(self._dir, "bootstraps.gz"))
        n, row_bytes = samples.shape[0], samples.shape[1] * samples.element_size()
        step = max(1, self.ROWS_BYTES // max(row_bytes, 1))
        for r0 in range(0, n, step):
            self._gz.write(samples[r0:r0 + step])
        self.written += n
        if self._log:
            self._log(0, f"wrote {self.written} bootstraps")
        return True

    def close(self):
        if self._f is not None:
            self._f.close(); self._f = None
        if self._gz is not None:
            gz, self._gz = self._gz, None
            self.last_result = gz.close()
