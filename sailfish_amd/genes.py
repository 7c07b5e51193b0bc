"""Gene-level aggregation of quant.sf -- host mirror of sailfish::utils::readTranscriptToGeneMap
(src/SailfishUtils.cpp:438-507), TranscriptGeneMap::geneName (include/TranscriptGeneMap.hpp:94-140),
aggregateEstimatesToGeneLevel (src/SailfishUtils.cpp:929-1037) and generateGeneLevelEstimates (:1039-1088), the
`--geneMap` post-processing step of `sailfish quant`.

aggregate_estimates_to_gene_level is the host restatement: it reads the PRINTED quant.sf back (so the 6-significant-digit
values), row by row.  aggregate_columns is the product path of `quantify(..., gene_map=...)`: the same file from the columns
where they lie on the device (sfgpu_genes_aggregate rounds them to their printed values, folds the genes with the function
of csrc/genefold.h and sfgpu_genes_write_text formats the rows), byte for byte; only the name lookup (vectorised,
TranscriptGeneMap.gene_ids_of) and the comment lines stay on the host.  The arithmetic is restated literally,
including two quirks a drop-in must keep:
  * totalTPM accumulates the RUNNING gene sum (`totalTPM += expVals[tpmIdx]` after the add, :1004-1009), so the
    TPM-weighted gene lengths are weighted by tpm_i / (sum of prefix sums), not by tpm_i / sum;
  * a transcript absent from the map is looked up with lower_bound and no equality test (:94-99): it lands on the
    next name in sorted order, and is "its own gene" only past the last name.
Lines of the output are in first-appearance order of the genes (the reference iterates an unordered_map: any order).
The GTF form of the map (`--geneMap x.gtf`, transcriptGeneMapFromGTF, :322-436) goes through libgff's GffReader in the
reference -- a third-party library that is not in the reference tree (CMakeLists.txt:408-419 fetches it), so its record
handling is restated from its use there: every record that carries a transcript_id makes (or extends) a transcript;
the grouping key is gene_id, gene_name, or any attribute named by `agg_key`; transcripts are ordered by name, genes
numbered by first appearance in that order.  Parity unpinned for this reader (no reference vector exists for it)."""
import bisect
import ctypes as C
import os

import numpy as np

from .writer import fmt_g

DENORM_MIN = 4.9406564584124654e-324


class TranscriptGeneMap:
    """readTranscriptToGeneMap (:438-507): `transcript gene` pairs, whitespace separated; names sorted."""

    def __init__(self, pairs):
        gene_id, gene_names, t2g_unordered, names = {}, [], [], []
        for t, g in pairs:
            if g not in gene_id:
                gene_id[g] = len(gene_names); gene_names.append(g)
            names.append(t); t2g_unordered.append(gene_id[g])
        order = sorted(range(len(names)), key=lambda i: names[i])         # std::sort on the names (stable enough: ties keep any order)
        self.transcript_names = [names[i] for i in order]
        self.t2g = [t2g_unordered[i] for i in order]
        self.gene_names = gene_names

    @classmethod
    def from_file(cls, path):
        toks = open(path).read().split()                                  # `ifile >> transcript >> gene` until it fails
        return cls(list(zip(toks[0::2], toks[1::2])))

    @classmethod
    def from_gtf(cls, path, agg_key="gene_id"):
        """transcriptGeneMapFromGTF (src/SailfishUtils.cpp:322-436).  GFF2/GTF records: 9 tab-separated columns, the last
        one `key "value"; key "value"; ...`; lines starting with # are comments."""
        first_key = {}                                                    # transcript_id -> value of the grouping key (first seen)
        for line in open(path):
            if not line.strip() or line.startswith("#"):
                continue
            cols = line.rstrip("\n").split("\t")
            if len(cols) < 9:
                continue
            attrs = {}
            for field in cols[8].split(";"):
                field = field.strip()
                if not field:
                    continue
                k, _, v = field.partition(" ")
                attrs.setdefault(k, v.strip().strip('"'))
            t = attrs.get("transcript_id")
            if not t:
                continue                                                  # gene records and the like: not a transcript (isTranscript())
            if t not in first_key or first_key[t] is None:
                first_key[t] = attrs.get(agg_key, first_key.get(t))
        obj = cls.__new__(cls)
        gene_id, obj.gene_names, obj.transcript_names, obj.t2g = {}, [], [], []
        for t in sorted(first_key):                                       # std::sort by strcmp on the transcript ids (:392-395)
            g = first_key[t] if first_key[t] is not None else ""
            if g not in gene_id:
                gene_id[g] = len(obj.gene_names); obj.gene_names.append(g)
            obj.transcript_names.append(t); obj.t2g.append(gene_id[g])
        return obj

    def num_transcripts(self): return len(self.transcript_names)
    def num_genes(self): return len(self.gene_names)

    def gene_name(self, transcript_name):
        i = bisect.bisect_left(self.transcript_names, transcript_name)   # findTranscriptID: lower_bound, no equality test
        return self.gene_names[self.t2g[i]] if i < len(self.transcript_names) else transcript_name

    def _arrays(self):
        """The map as numpy arrays, built once and kept while the three lists are the same objects of the same lengths:
        (sorted transcript names, t2g, gene names, gene names sorted, their positions in gene_names)."""
        key = (id(self.transcript_names), len(self.transcript_names), id(self.gene_names), len(self.gene_names), id(self.t2g), len(self.t2g))
        cache = getattr(self, "_np_cache", None)
        if cache is None or cache[0] != key:
            gnames = np.asarray(self.gene_names, dtype=np.str_).reshape(-1)
            order = np.argsort(gnames, kind="stable")
            cache = (key, (np.asarray(self.transcript_names, dtype=np.str_).reshape(-1), np.asarray(self.t2g, np.int64).reshape(-1),
                           gnames, gnames[order], order))
            self._np_cache = cache
        return cache[1]

    def _lookup(self, names):
        """(queries, positions): the names as a numpy string array and lower_bound of each in transcript_names.  Code-point
        order of fixed-width unicode arrays, which is the byte-wise order of the UTF-8 names (and Python's str order)."""
        q = np.asarray(names, dtype=np.str_).reshape(-1)
        return q, np.searchsorted(self._arrays()[0], q, side="left")

    def gene_names_of(self, names):
        """gene_name of every name in `names`, without a per-name Python loop: lower_bound with no equality test; past the
        last name a transcript is its own gene.  Returns a list of str."""
        q, pos = self._lookup(names)
        if len(q) == 0:
            return []
        tnames, t2g, gnames, _, _ = self._arrays()
        n = len(tnames)
        if n == 0:
            return q.tolist()
        genes = gnames[t2g[np.minimum(pos, n - 1)]]
        width = max(q.dtype.itemsize, genes.dtype.itemsize, 4) // 4
        return np.where(pos < n, genes.astype(f"U{width}"), q.astype(f"U{width}")).tolist()

    def gene_ids_of(self, names):
        """The gene of every name as an id, keyed by the gene's NAME as the host dict is: (ids uint32[len(names)], table) with
        table[id] the name.  Ids below num_genes() are the map's genes; a transcript that is its own gene takes the id of the map
        gene of that name when there is one, otherwise a new id (one per distinct name, appended to the table)."""
        q, pos = self._lookup(names)
        tnames, t2g, _, gsorted_names, gorder = self._arrays()
        n, G = len(tnames), len(self.gene_names)
        ids = np.zeros(len(q), np.int64)
        table = list(self.gene_names)
        inside = pos < n
        if n:
            ids[inside] = t2g[pos[inside]]
        own = np.flatnonzero(~inside)
        if len(own):
            uniq, inv = np.unique(q[own], return_inverse=True)
            hit = np.zeros(len(uniq), bool)
            uid = np.zeros(len(uniq), np.int64)
            if G:
                at = np.minimum(np.searchsorted(gsorted_names, uniq), G - 1)
                hit = gsorted_names[at] == uniq
                uid[hit] = gorder[at[hit]]                                 # a map gene has that name: the transcript joins it
            uid[~hit] = G + np.arange(int((~hit).sum()), dtype=np.int64)   # otherwise a new id per distinct own name
            ids[own] = uid[inv.reshape(-1)]
            table += uniq[~hit].tolist()
        return ids.astype(np.uint32), table


def aggregate_estimates_to_gene_level(tgm: TranscriptGeneMap, quant_path: str) -> str:
    """aggregateEstimatesToGeneLevel (:929-1037): writes <quant_path minus extension>.genes.sf, returns its path."""
    comments, gene_exps, header = [], {}, True
    for line in open(quant_path).read().split("\n"):
        if not line.strip():
            continue
        if line.lstrip()[0] == "#":
            comments.append(line)
        elif header:
            comments.append(line); header = False                         # the header line is kept as a comment (:970-973)
        else:
            toks = line.split()
            if len(toks) < 3:
                raise ValueError("Any expression line must contain at least 3 tokens")
            rec = (toks[0], float(int(toks[1])), float(toks[2]), [float(x) for x in toks[3:]])   # stoi, stod, stod...
            gene_exps.setdefault(tgm.gene_name(rec[0]), []).append(rec)
    out_path = os.path.splitext(quant_path)[0] + ".genes.sf"
    with open(out_path, "w") as out:
        for c in comments:
            out.write(c + "\n")
        for gene, recs in gene_exps.items():
            ne = len(recs[0][3])
            exp_vals = [0.0] * ne
            total_tpm = 0.0
            for _, _, _, vals in recs:
                for i in range(ne):
                    exp_vals[i] += vals[i]
                total_tpm += exp_vals[0]                                  # the running sum, as in the reference
            gene_len = gene_eff = 0.0
            if total_tpm > DENORM_MIN:
                for _, length, eff, vals in recs:
                    frac = vals[0] / total_tpm
                    gene_len += length * frac; gene_eff += eff * frac
            else:
                frac = 1.0 / len(recs)
                for _, length, eff, _ in recs:
                    gene_len += length * frac; gene_eff += eff * frac
            out.write("\t".join([gene, fmt_g(gene_len), fmt_g(gene_eff)] + [fmt_g(v) for v in exp_vals]) + "\n")
    return out_path


def _to_device(a, dtype, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype).copy()).to(device)


def aggregate_device(gene_of_row, n_gene_ids, length, eff, tpm, num_reads, as_printed=True):
    """sfgpu_genes_aggregate on device columns, behind torch's current stream: gene_of_row (32-bit integer device tensor of
    ids below n_gene_ids), length (32-bit integers), eff / tpm / num_reads (float64).  Returns (gene_id, length, eff, tpm,
    num_reads, result dict): the output lines as device tensors (gene_id int32 holding uint32 bits, the rest float64)."""
    import torch

    from . import _lib
    n = eff.numel()
    for t in (gene_of_row, length):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and not t.is_floating_point() and t.element_size() == 4 and t.numel() == n):
            raise TypeError("gene_of_row / length: expected device tensors of 32-bit integers, one per row")
    for t in (eff, tpm, num_reads):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.numel() == n):
            raise TypeError("eff / tpm / num_reads: expected float64 device tensors, one per row")
    cap = max(min(n, int(n_gene_ids)), 1)
    gid = torch.zeros(cap, dtype=torch.int32, device=eff.device)
    outs = [torch.zeros(cap, dtype=torch.float64, device=eff.device) for _ in range(4)]
    res = _lib.GenesResult()
    with torch.cuda.device(eff.device):
        _lib.check(_lib.lib().sfgpu_genes_aggregate(_lib.ptr(gene_of_row.contiguous()), _lib.ptr(length.contiguous()), _lib.ptr(eff.contiguous()),
                                                    _lib.ptr(tpm.contiguous()), _lib.ptr(num_reads.contiguous()), n, int(n_gene_ids),
                                                    1 if as_printed else 0, _lib.ptr(gid), *[_lib.ptr(o) for o in outs], C.byref(res),
                                                    _lib.current_stream_ptr()))
    g = int(res.n_genes)
    return (gid[:g],) + tuple(o[:g] for o in outs) + (res.as_dict(),)


def write_gene_rows(fileobj, table, gene_id, length, eff, tpm, num_reads, chunk_bytes=0):
    """The rows of quant.genes.sf, formatted on the device (sfgpu_genes_write_text), into the binary file object `fileobj`:
    row g is named table[gene_id[g]].  `table`: a list of names, or a (uint8 blob, 64-bit offsets) pair of device tensors.
    Returns the sfgpu_quant_write_result as a dict.  An exception of fileobj.write stops the writer and is raised again here."""
    import torch

    from . import _lib, quantfile
    if isinstance(table, tuple):
        blob, off = table
    else:
        b, o = quantfile.names_blob(table)
        blob = _to_device(np.frombuffer(b, np.uint8), np.uint8, eff.device)
        off = _to_device(o, np.int64, eff.device)
    raised = []

    def sink(addr, n, _user):
        try:                                   # nothing may unwind through the C frame
            fileobj.write(memoryview((C.c_char * n).from_address(addr)))
            return 0
        except BaseException as e:             # noqa: BLE001  (re-raised below)
            raised.append(e)
            return 1

    res = _lib.QuantWriteResult()
    with torch.cuda.device(eff.device):
        rc = _lib.lib().sfgpu_genes_write_text(_lib.ptr(blob) if blob.numel() else None, _lib.ptr(off.contiguous()), off.numel() - 1,
                                               _lib.ptr(gene_id.contiguous()), _lib.ptr(length.contiguous()), _lib.ptr(eff.contiguous()),
                                               _lib.ptr(tpm.contiguous()), _lib.ptr(num_reads.contiguous()), gene_id.numel(), int(chunk_bytes),
                                               _lib.TEXT_SINK(sink) if fileobj is not None else _lib.TEXT_SINK(0), None, C.byref(res),
                                               _lib.current_stream_ptr())
    if raised:
        raise raised[0]
    _lib.check(rc)
    return res.as_dict()


QUANT_HEADER = "Name\tLength\tEffectiveLength\tTPM\tNumReads"


def aggregate_columns(tgm: TranscriptGeneMap, names, length, eff, tpm, num_reads, out_path: str, comments=(QUANT_HEADER,),
                      as_printed=True, chunk_bytes=0):
    """quant.genes.sf at `out_path` from the columns of quant.sf where they lie, without reading the file back: the bytes
    aggregate_estimates_to_gene_level writes from the quant.sf that quantfile.write_file writes from the same columns.
    `names`: the transcript names (host list, no whitespace inside a name, as the reference's reader requires); `length`:
    32-bit integer device tensor; eff / tpm / num_reads: float64 device tensors.  `comments`: the lines the host function
    would copy from quant.sf, its header line included.  The names are looked up and factorised to ids on the host (gene_ids_of),
    the genes are folded and the rows formatted on the device; the comment lines are written here.
    Returns {"aggregate": sfgpu_genes_result, "write": sfgpu_quant_write_result} as dicts."""
    ids, table = tgm.gene_ids_of(names)
    if len(ids) != eff.numel():
        raise ValueError(f"{len(ids)} names for {eff.numel()} rows")
    d_ids = _to_device(ids, np.int32, eff.device)
    gid, g_len, g_eff, g_tpm, g_nr, agg = aggregate_device(d_ids, len(table), length, eff, tpm, num_reads, as_printed=as_printed)
    with open(out_path, "wb") as f:
        for c in comments:
            f.write(c.encode("utf-8") + b"\n")
        wr = write_gene_rows(f, table, gid, g_len, g_eff, g_tpm, g_nr, chunk_bytes) if agg["n_genes"] else {}
    return {"aggregate": agg, "write": wr}


def generate_gene_level_estimates(gene_map_path: str, est_dir: str, agg_key: str = "gene_id", columns=None) -> str:
    """generateGeneLevelEstimates (:1039-1088): a map whose extension is .gtf is read as GTF, anything else as the
    two-column format.  `columns`, when given, is (names, length, eff, tpm, num_reads) as aggregate_columns takes them --
    the columns the caller has just written to <est_dir>/quant.sf: the genes are then folded on the device from those
    (aggregate_columns) instead of from the file read back, with the same bytes in quant.genes.sf."""
    if os.path.splitext(gene_map_path)[1] == ".gtf":
        tgm = TranscriptGeneMap.from_gtf(gene_map_path, agg_key)
    else:
        tgm = TranscriptGeneMap.from_file(gene_map_path)
    if columns is not None:
        out_path = os.path.join(est_dir, "quant.genes.sf")
        aggregate_columns(tgm, *columns, out_path)
        return out_path
    est = os.path.join(est_dir, "quant.sf")
    if not os.path.exists(est):
        raise ValueError(f"Attempting to compute gene-level esimtates, but could not \nfind isoform-level file {est}")
    return aggregate_estimates_to_gene_level(tgm, est)
