"""Gene-level aggregation of quant.sf -- host mirror of sailfish::utils::readTranscriptToGeneMap
(src/SailfishUtils.cpp:438-507), TranscriptGeneMap::geneName (include/TranscriptGeneMap.hpp:94-140),
aggregateEstimatesToGeneLevel (src/SailfishUtils.cpp:929-1037) and generateGeneLevelEstimates (:1039-1088), the
`--geneMap` post-processing step of `sailfish quant`.

aggregate_estimates_to_gene_level is the host restatement: it reads the PRINTED quant.sf back (so the 6-significant-digit
values), row by row.  aggregate_columns is the product path of `quantify(..., gene_map=...)`: the same file from the columns
where they lie on the device (sfgpu_genes_aggregate rounds them to their printed values, folds the genes with the function
of csrc/genefold.h and sfgpu_genes_write_text formats the rows), byte for byte.  With a DeviceGeneMap -- the map file read on
the device (sfgpu_gmap_*, csrc/genemap.hip; the rules of the two readers below restated in csrc/gtffmt.h) -- the names are
joined there as well (sfgpu_gmap_lookup) and only the comment lines stay on the host; with a TranscriptGeneMap the name lookup
(vectorised, TranscriptGeneMap.gene_ids_of) is host work.  The arithmetic is restated literally,
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
import collections
import ctypes as C
import gzip
import os
import tempfile
import time

import numpy as np

from .writer import fmt_g

DENORM_MIN = 4.9406564584124654e-324


def _gtf_attrs(col8):
    """column 9 of a GTF record, `key "value"; key "value"; ...` -> {key: value}, the first value of a key kept"""
    attrs = {}
    for field in col8.split(";"):
        field = field.strip()
        if not field:
            continue
        k, _, v = field.partition(" ")
        attrs.setdefault(k, v.strip().strip('"'))
    return attrs


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
            attrs = _gtf_attrs(cols[8])
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


EXON_STATUS = {0: "placed", 1: "absent from the annotation", 2: "exons on more than one chromosome or strand", 3: "a strand other than + or -",
               4: "two exons overlap"}
Placement = collections.namedtuple("Placement", "status chrom strand exon_off exon_start exon_len n_chrom chrom_names")


class ExonModel:
    """The exon structure of an annotation's transcripts, for the genome coverage track (csrc/covgfmt.h's MODEL).  from_gtf reads it on
    the host, once a run; for_names joins it to a run's transcripts.
    chrom_names   the chromosomes' names (bytes, as the file has them), numbered in BYTEWISE order -- the order `LC_ALL=C sort -k1,1`
                  leaves, so the coverage file comes out sorted the way bedGraphToBigWig wants it
    transcripts   {transcript_id bytes: (status, chrom id, strand +1 / -1 / 0, [(start0, len), ...] in transcript order)}; the blocks
                  only where status is 0 (EXON_STATUS)"""

    def __init__(self, chrom_names, transcripts):
        self.chrom_names, self.transcripts = list(chrom_names), dict(transcripts)

    @classmethod
    def from_gtf(cls, path):
        """Plain or gzip (by its magic bytes).  gtffmt.h's line rules: lines that start with # and lines of fewer than 9 tab-separated
        columns are skipped, a \\r before the \\n is dropped.  A line counts iff column 3 is exactly `exon` and column 9 carries a
        transcript_id that is not empty (TranscriptGeneMap.from_gtf's fields).  Column 1, the chromosome, must not be empty; columns
        4 and 5 are decimal with 1 <= start <= end <= 4294967295; anything else is a ValueError naming the 1-based line.  A
        transcript's exons are sorted by start and, on -, reversed; its status is 2 where they name more than one chromosome or
        strand, else 3 where the strand is neither + nor -, else 4 where two of them overlap (identical ones included; touching
        ones are fine), else 0."""
        with open(path, "rb") as f:
            magic = f.read(2)
        with (gzip.open(path, "rb") if magic == b"\x1f\x8b" else open(path, "rb")) as f:
            data = f.read()
        seen = {}                                                         # transcript_id -> [set of (chrom, strand), [(start0, len)]]
        for no, line in enumerate(data.split(b"\n"), 1):
            if line.endswith(b"\r"):
                line = line[:-1]
            if line.startswith(b"#"):
                continue
            cols = line.split(b"\t")
            if len(cols) < 9 or cols[2] != b"exon":
                continue
            t = _gtf_attrs(cols[8].decode("latin-1")).get("transcript_id")
            if not t:
                continue
            if not cols[0]:
                raise ValueError(f"{path}: line {no}: an exon without a chromosome name")
            if not (cols[3].isdigit() and cols[4].isdigit() and cols[3].isascii() and cols[4].isascii()):
                raise ValueError(f"{path}: line {no}: the exon's start and end must be decimal integers")
            a, b = int(cols[3]), int(cols[4])
            if not 1 <= a <= b <= 4294967295:
                raise ValueError(f"{path}: line {no}: an exon needs 1 <= start <= end <= 4294967295, not {a} and {b}")
            where, blocks = seen.setdefault(t.encode("latin-1"), [set(), []])
            where.add((cols[0], cols[6]))
            blocks.append((a - 1, b - a + 1))
        chrom_names = sorted({c for where, _ in seen.values() for c, _ in where})
        chrom_id = {c: i for i, c in enumerate(chrom_names)}
        transcripts = {}
        for t, (where, blocks) in seen.items():
            (c, strand), blocks = next(iter(where)), sorted(blocks)
            if len(where) > 1:
                transcripts[t] = (2, -1, 0, [])
            elif strand not in (b"+", b"-"):
                transcripts[t] = (3, -1, 0, [])
            elif any(x[0] + x[1] > y[0] for x, y in zip(blocks, blocks[1:])):
                transcripts[t] = (4, -1, 0, [])
            else:
                transcripts[t] = (0, chrom_id[c], 1 if strand == b"+" else -1, blocks if strand == b"+" else blocks[::-1])
        return cls(chrom_names, transcripts)

    def for_names(self, names):
        """The model joined to a run's transcripts by exact byte equality of the names (str as UTF-8), the gene map's rule: a transcript
        the annotation does not have gets status 1.  -> Placement(status uint8[M], chrom int32[M], strand int8[M], exon_off int64[M + 1],
        exon_start uint32[E], exon_len uint32[E], n_chrom, chrom_names): what sfgpu_covg_open and hits.coverage_genome_host take."""
        M = len(names)
        status, chrom, strand, off = np.ones(M, np.uint8), np.full(M, -1, np.int32), np.zeros(M, np.int8), np.zeros(M + 1, np.int64)
        starts, lens = [], []
        for i, n in enumerate(names):
            rec = self.transcripts.get(n.encode("utf-8") if isinstance(n, str) else bytes(n))
            if rec is not None:
                status[i], chrom[i], strand[i] = rec[:3]
                starts += [b[0] for b in rec[3]]
                lens += [b[1] for b in rec[3]]
            off[i + 1] = len(starts)
        return Placement(status, chrom, strand, off, np.array(starts, np.uint32), np.array(lens, np.uint32), len(self.chrom_names), list(self.chrom_names))

    def chrom_lengths(self, sizes=None):
        """LN of every chromosome, in the order of chrom_names, for the @SQ lines of a genome-coordinate mappings file.  sizes: the path
        of a chrom.sizes / .fai-style file -- the first two tab-separated columns of every line that is not empty are the name (bytes,
        matched exactly) and the decimal length; a chromosome of the model that the file does not name is a ValueError, as is a
        length that is no decimal integer.  Without it LN is the furthest exon end of a placed transcript on that chromosome (1 where
        none is placed there): a LOWER bound of the chromosome's length, which viewers accept; give `sizes` where a tool compares LN
        with its own genome."""
        if sizes is not None:
            table = {}
            with open(sizes, "rb") as f:
                for no, line in enumerate(f.read().split(b"\n"), 1):
                    line = line[:-1] if line.endswith(b"\r") else line
                    if not line:
                        continue
                    cols = line.split(b"\t")
                    if len(cols) < 2 or not (cols[1].isdigit() and cols[1].isascii()):
                        raise ValueError(f"{sizes}: line {no}: expected a name, a tab and a decimal length")
                    table.setdefault(cols[0], int(cols[1]))
            missing = [c for c in self.chrom_names if c not in table]
            if missing:
                raise ValueError(f"{sizes}: no length for chromosome {missing[0].decode('utf-8', 'replace')!r} of the annotation ({len(missing)} missing)")
            return [table[c] for c in self.chrom_names]
        ends = [1] * len(self.chrom_names)
        for status, c, _, blocks in self.transcripts.values():
            if status == 0:
                ends[c] = max([ends[c]] + [gs + n for gs, n in blocks])
        return ends


HOST_REASONS = {1: "a byte >= 0x80", 2: "a NUL byte", 4: "a '\\r' that is not followed by '\\n'", 8: "a name longer than 256 bytes"}


class _TimedReader:
    """readinto of a binary stream, with the seconds it took"""

    def __init__(self, f):
        self.f, self.seconds = f, 0.0

    def readinto(self, b):
        t0 = time.perf_counter()
        n = self.f.readinto(b)
        self.seconds += time.perf_counter() - t0
        return n


class DeviceGeneMap:
    """A --geneMap file as tables on the device: the sorted transcript names, t2g and the gene names of the TranscriptGeneMap that
    from_gtf / from_file give for the same file (to_host() returns exactly that), built without a per-line host loop
    (sfgpu_gmap_add_text_host / _device, sfgpu_gmap_finish) and joined to transcript names without host strings (lookup).

    from_path: an extension .gtf selects the GTF rules, anything else the two-column rules (generate_gene_level_estimates' rule); a
    gzip file is detected by its magic bytes and the rules are then chosen from the extension under a trailing .gz.  The file is
    read in blocks of block_bytes (at least 64; bytes of the file as stored) and the unconsumed tail is carried by the carriers of
    `readfile`: BlockCarry for a plain file and for a gzip file inflated by Python's gzip, DeviceInflate / DeviceGunzip for one
    inflated on the device, with this class's parse callback in place of ReadFile's.  `inflate` is ReadFile's: "auto" takes the
    device for a BGZF file and the host for any other gzip file.
    A file that holds what the device rules do not parse (csrc/gtffmt.h: a non-ASCII byte, a NUL, a lone CR, a name longer than
    256 bytes) is read by the host reader and uploaded (sfgpu_gmap_from_host): stats["reader"] is "host" and stats["reason"] says
    why; otherwise stats["reader"] is "device".  stats also holds the seconds spent reading the file (read_s), the device times
    of the calls (ms_copy, ms_kernels, ms_finish), calls, bytes, lines, records, sort_rounds."""

    MIN_BLOCK = 64

    def __init__(self, handle, device, is_gtf, stats):
        self._h, self.device, self.is_gtf, self.stats = handle, device, is_gtf, stats
        self._host = self._tables = None

    # ---- reading
    @classmethod
    def from_path(cls, path, agg_key="gene_id", device="cuda", block_bytes=32 << 20, inflate="auto"):
        import torch

        from . import _lib, readfile
        if inflate not in ("auto", "host", "device"):
            raise ValueError("inflate must be 'auto', 'host' or 'device'")
        if int(block_bytes) < cls.MIN_BLOCK:
            raise ValueError(f"block_bytes must be at least {cls.MIN_BLOCK}")
        path = str(path)
        device = torch.device(device)
        with open(path, "rb") as f:
            head = f.read(4096)
        gzipped = head[:2] == b"\x1f\x8b"
        stem = path[:-3] if gzipped and path.endswith(".gz") else path
        is_gtf = os.path.splitext(stem)[1] == ".gtf"
        bgzf = gzipped and readfile.bgzf_member_bytes(head) is not None
        where = None if not gzipped else "device" if inflate == "device" or (inflate == "auto" and bgzf) else "host"
        L = _lib.lib()
        key = agg_key.encode("utf-8")
        h = C.c_void_p()
        with torch.cuda.device(device):
            _lib.check(L.sfgpu_gmap_open(C.byref(h), 0 if is_gtf else 1, key, len(key)))
        reader = _GmapReader(L, h, device, path)
        try:
            if where == "device":
                f = open(path, "rb", buffering=0)
                timed = _TimedReader(f)
                carry = (readfile.DeviceInflate if bgzf else readfile.DeviceGunzip)(reader, timed, block_bytes)
                reader._carry = carry
                try:
                    while carry.next(1 << 62) is not None:
                        pass
                except _NeedsHost:
                    pass
                finally:
                    carry.close(); f.close()
            else:
                f = gzip.open(path, "rb") if gzipped else open(path, "rb", buffering=0)
                timed = _TimedReader(f)
                carry = readfile.BlockCarry(timed, block_bytes, path)
                try:
                    while carry.next(reader.parse_host, 1 << 62) is not None:
                        pass
                except _NeedsHost:
                    pass
                finally:
                    f.close()
            stats = reader.stats
            stats.update(read_s=timed.seconds, inflate=where)
            if reader.needs_host:
                with torch.cuda.device(device):
                    L.sfgpu_gmap_close(h)
                h = None
                return cls._from_host_reader(path, is_gtf, agg_key, gzipped, device, stats, reader.needs_host)
            res = _lib.GmapResult()
            with torch.cuda.device(device):
                _lib.check(L.sfgpu_gmap_finish(h, C.byref(res), _lib.current_stream_ptr()))
            stats.update(reader="device", reason=None, ms_finish=res.ms_kernels, sort_rounds=int(res.sort_rounds), n_records=int(res.n_records))
            out = cls(h, device, is_gtf, stats)
            out._sizes = (int(res.n_transcripts), int(res.n_genes), int(res.tname_bytes), int(res.gname_bytes))
            h = None
            return out
        finally:
            if h is not None:
                with torch.cuda.device(device):
                    L.sfgpu_gmap_close(h)

    @classmethod
    def _from_host_reader(cls, path, is_gtf, agg_key, gzipped, device, stats, flags):
        tmp = None
        try:
            if gzipped:                                                   # the host readers open plain files
                with gzip.open(path, "rb") as f, tempfile.NamedTemporaryFile(suffix=".gtf" if is_gtf else ".tsv", delete=False) as out:
                    tmp = out.name
                    out.write(f.read())
            src = tmp or path
            tgm = TranscriptGeneMap.from_gtf(src, agg_key) if is_gtf else TranscriptGeneMap.from_file(src)
        finally:
            if tmp:
                os.unlink(tmp)
        out = cls.from_host_map(tgm, device)
        out.is_gtf = is_gtf
        out.stats = dict(stats, reader="host", reason="; ".join(v for k, v in HOST_REASONS.items() if flags & k))
        return out

    @classmethod
    def from_host_map(cls, tgm, device="cuda"):
        """the tables of a TranscriptGeneMap uploaded (sfgpu_gmap_from_host); to_host() returns `tgm` itself"""
        import torch

        from . import _lib, quantfile
        device = torch.device(device)
        tb, to = quantfile.names_blob(tgm.transcript_names)
        gb, go = quantfile.names_blob(tgm.gene_names)
        t2g = np.ascontiguousarray(tgm.t2g, dtype=np.uint32)
        h = C.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().sfgpu_gmap_from_host(C.byref(h), tb, _lib.ptr(to), _lib.ptr(t2g), len(tgm.transcript_names), gb, _lib.ptr(go),
                                                       len(tgm.gene_names)))
        out = cls(h, device, None, dict(reader="host", reason=None))
        out._sizes = (len(tgm.transcript_names), len(tgm.gene_names), len(tb), len(gb))
        out._host = tgm
        return out

    # ---- the tables
    def num_transcripts(self): return self._sizes[0]
    def num_genes(self): return self._sizes[1]

    def tables(self):
        """(tnames uint8, tname_off int64 [T + 1], t2g int32 holding uint32 bits [T], gnames uint8, gname_off int64 [G + 1]) on the
        device, copied out of the handle once"""
        import torch

        from . import _lib
        if self._h is None:
            raise ValueError("the gene map is closed")
        if self._tables is None:
            T, G, tb, gb = self._sizes
            mk = lambda n, dt: torch.empty(max(n, 1), dtype=dt, device=self.device)
            tn, to, t2g, gn, go = mk(tb, torch.uint8), mk(T + 1, torch.int64), mk(T, torch.int32), mk(gb, torch.uint8), mk(G + 1, torch.int64)
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().sfgpu_gmap_export(self._h, _lib.ptr(tn), _lib.ptr(to), _lib.ptr(t2g), _lib.ptr(gn), _lib.ptr(go),
                                                        _lib.current_stream_ptr()))
            self._tables = (tn[:tb], to, t2g[:T], gn[:gb], go)
        return self._tables

    def gene_table(self):
        """the gene names as the (blob, offsets) pair write_gene_rows takes"""
        t = self.tables()
        return t[3], t[4]

    def to_host(self):
        """the TranscriptGeneMap of the same file"""
        if self._host is None:
            tn, to, t2g, gn, go = (x.cpu().numpy() for x in self.tables())
            cut = lambda blob, off: [blob[a:b].tobytes().decode("utf-8") for a, b in zip(off[:-1].tolist(), off[1:].tolist())]
            m = TranscriptGeneMap.__new__(TranscriptGeneMap)
            m.transcript_names, m.gene_names = cut(tn, to), cut(gn, go)
            m.t2g = t2g.view(np.uint32).astype(np.int64).tolist()
            self._host = m
        return self._host

    def lookup(self, names):
        """findTranscriptID for every row name.  `names`: the (uint8 blob, 64-bit offsets) pair of device tensors that
        Transcripts.name_blob() returns.  -> (gene_of_row: int32 device tensor holding uint32 bits, n_past): lower_bound with no
        equality test; the n_past rows past the last name hold 0xFFFFFFFF."""
        import torch

        from . import _lib
        if self._h is None:
            raise ValueError("the gene map is closed")
        blob, off = names
        n = off.numel() - 1
        out = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        n_past = C.c_uint64(0)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().sfgpu_gmap_lookup(self._h, _lib.ptr(blob.contiguous()) if blob.numel() else None, _lib.ptr(off.contiguous()), n,
                                                    _lib.ptr(out), C.byref(n_past), _lib.current_stream_ptr()))
        return out[:n], int(n_past.value)

    def close(self):
        if self._h is not None:
            import torch

            from . import _lib
            with torch.cuda.device(self.device):
                _lib.lib().sfgpu_gmap_close(self._h)
            self._h = self._tables = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001  (interpreter shutdown)
            pass


class _NeedsHost(Exception):
    """raised out of the block loop by the first call that reports needs_host: nothing more of the file is read for the device"""


class _GmapReader:
    """what the carriers of `readfile` drive: the parse callbacks over one sfgpu_gmap handle (and the attributes DeviceCarry reads
    from its owner)"""

    def __init__(self, L, handle, device, path):
        self._L, self._h, self.device, self.path = L, handle, device, path
        self._carry = None
        self.needs_host = 0
        self.stats = dict(calls=0, bytes_parsed=0, n_lines=0, ms_copy=0.0, ms_kernels=0.0, ms_inflate=0.0, bytes_compressed=0, members=0,
                          chunks=0, candidates=0, false_starts=0, ms_find=0.0, ms_decode=0.0, ms_propagate=0.0, ms_emit=0.0)

    def _done(self, rc, res, n):
        from . import _lib, readfile
        if rc == _lib.ERR_RANGE and res.consumed == 0 and n <= readfile.MAX_TEXT:
            return readfile.Parsed(0, 0)                                   # no line ends in this text: the carrier presents more
        _lib.check(rc)
        self.needs_host |= int(res.needs_host)
        for k, v in (("calls", 1), ("bytes_parsed", int(res.consumed)), ("n_lines", int(res.n_lines)), ("ms_copy", res.ms_copy),
                     ("ms_kernels", res.ms_kernels)):
            self.stats[k] += v
        if self.needs_host:
            raise _NeedsHost()                                             # the host reader takes the whole file: read no further
        return readfile.Parsed(int(res.n_lines), int(res.consumed))

    def parse_host(self, text, final, _max_reads):
        import torch

        from . import _lib
        res = _lib.GmapAddResult()
        with torch.cuda.device(self.device):
            rc = self._L.sfgpu_gmap_add_text_host(self._h, _lib.ptr(text), int(text.size), int(final), C.byref(res), _lib.current_stream_ptr())
        return self._done(rc, res, int(text.size))

    def _parse_device(self, text, lo, hi, final, _max_reads, _records):
        import torch

        from . import _lib
        n = hi - lo
        res = _lib.GmapAddResult()
        with torch.cuda.device(self.device):
            if lo % 16:                                                    # the parser wants its text at a 16-byte boundary
                text[:n] = text[lo:hi].clone()
                self._carry.lo, self._carry.hi, lo, hi = 0, n, 0, n
            view = text[lo:]
            rc = self._L.sfgpu_gmap_add_text_device(self._h, _lib.ptr(view), n, view.numel(), int(final), C.byref(res), _lib.current_stream_ptr())
        out = self._done(rc, res, n)
        if out.n_reads and not final:
            self._carry.starved = True                                     # what is left holds no line end: inflate before the next call
        return out


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


def _names_of_blob(names):
    """the host list of a (blob, offsets) pair of device tensors"""
    blob, off = (x.cpu().numpy() for x in names)
    return [blob[a:b].tobytes().decode("utf-8") for a, b in zip(off[:-1].tolist(), off[1:].tolist())]


def _device_gene_ids(dmap, names, device):
    """(gene id of every row as a device tensor, gene table, number of ids) through a DeviceGeneMap"""
    if isinstance(names, tuple):
        pair = names
    else:
        from . import quantfile
        b, o = quantfile.names_blob(names)
        pair = (_to_device(np.frombuffer(b, np.uint8), np.uint8, device), _to_device(o, np.int64, device))
    ids, n_past = dmap.lookup(pair)
    if n_past == 0:
        return ids, dmap.gene_table(), dmap.num_genes()
    host_ids, table = dmap.to_host().gene_ids_of(names if not isinstance(names, tuple) else _names_of_blob(names))
    return _to_device(host_ids, np.int32, device), table, len(table)


def aggregate_columns(tgm, names, length, eff, tpm, num_reads, out_path: str, comments=(QUANT_HEADER,),
                      as_printed=True, chunk_bytes=0):
    """quant.genes.sf at `out_path` from the columns of quant.sf where they lie, without reading the file back: the bytes
    aggregate_estimates_to_gene_level writes from the quant.sf that quantfile.write_file writes from the same columns.
    `names`: the transcript names (host list, no whitespace inside a name, as the reference's reader requires); `length`:
    32-bit integer device tensor; eff / tpm / num_reads: float64 device tensors.  `comments`: the lines the host function
    would copy from quant.sf, its header line included.  The names are looked up and factorised to ids on the host (gene_ids_of),
    the genes are folded and the rows formatted on the device; the comment lines are written here.
    With a DeviceGeneMap the names are joined on the device (sfgpu_gmap_lookup); `names` is then best the (blob, offsets) pair of
    Transcripts.name_blob() (a host list is uploaded), and while no row lies past the map's last name -- the usual case -- no
    string touches the host: the gene table handed to the row writer is the map's device pair.  Rows past the last name are
    "their own gene", keyed by name as the host dict is: the ids are then resolved by gene_ids_of on the map's to_host().
    Returns {"aggregate": sfgpu_genes_result, "write": sfgpu_quant_write_result} as dicts."""
    if isinstance(tgm, DeviceGeneMap):
        d_ids, table, n_ids = _device_gene_ids(tgm, names, eff.device)
    else:
        if isinstance(names, tuple):
            names = _names_of_blob(names)
        ids, table = tgm.gene_ids_of(names)
        d_ids, n_ids = _to_device(ids, np.int32, eff.device), len(table)
    if d_ids.numel() != eff.numel():
        raise ValueError(f"{d_ids.numel()} names for {eff.numel()} rows")
    gid, g_len, g_eff, g_tpm, g_nr, agg = aggregate_device(d_ids, n_ids, length, eff, tpm, num_reads, as_printed=as_printed)
    with open(out_path, "wb") as f:
        for c in comments:
            f.write(c.encode("utf-8") + b"\n")
        wr = write_gene_rows(f, table, gid, g_len, g_eff, g_tpm, g_nr, chunk_bytes) if agg["n_genes"] else {}
    return {"aggregate": agg, "write": wr}


def generate_gene_level_estimates(gene_map_path: str, est_dir: str, agg_key: str = "gene_id", columns=None) -> str:
    """generateGeneLevelEstimates (:1039-1088): a map whose extension is .gtf is read as GTF, anything else as the
    two-column format.  `columns`, when given, is (names, length, eff, tpm, num_reads) as aggregate_columns takes them --
    the columns the caller has just written to <est_dir>/quant.sf: the map is then read on the device (DeviceGeneMap.from_path,
    which also takes a gzip-compressed map) and the genes are folded there from those columns (aggregate_columns) instead of
    from the file read back, with the same bytes in quant.genes.sf."""
    if columns is not None:
        dmap = DeviceGeneMap.from_path(gene_map_path, agg_key, device=columns[2].device)          # the map is read and joined on the device
        out_path = os.path.join(est_dir, "quant.genes.sf")
        with dmap:
            aggregate_columns(dmap, *columns, out_path)
        return out_path
    if os.path.splitext(gene_map_path)[1] == ".gtf":
        tgm = TranscriptGeneMap.from_gtf(gene_map_path, agg_key)
    else:
        tgm = TranscriptGeneMap.from_file(gene_map_path)
    est = os.path.join(est_dir, "quant.sf")
    if not os.path.exists(est):
        raise ValueError(f"Attempting to compute gene-level esimtates, but could not \nfind isoform-level file {est}")
    return aggregate_estimates_to_gene_level(tgm, est)
