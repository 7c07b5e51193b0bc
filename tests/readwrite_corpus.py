"""Batches of reads for the device read writer (csrc/readwfmt.h, csrc/readtext_write.hip), shared by tests/test_readwrite_cpu.py
and tests/test_gpu_readwrite.py.  Deterministic, a few KB each; what every batch must give is readfile.reads_text_host.

A case is a dict: seqs, quals (None: FASTA), names (None: generated), select (None: all), base (the index of record 0),
misaligned (every array is handed over as a view that starts at an odd byte: _odd) and error (None, or the (record, kind) the
statement names).  cases() is every named case, both formats unless its name says otherwise; random_case(i) is batch i of the
random ones."""
import numpy as np

TILE = 4096
N_RANDOM = 300
NAME_RUNS = (0, 1, 47, 48, 49, 63, 64, 65, 300)
BASE_RUNS = (0, 1, 47, 48, 49, 64, 4096, 10_000)
INDEX_BASES = (0, 9, 10, 99_999, 2 ** 32 + 5)
_BASES = np.frombuffer(b"ACGTN", np.uint8)
_NAME = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_.:/-", np.uint8)


def _seq(rng, n):
    return _BASES[rng.integers(0, 5, n)].tobytes()


def _qual(rng, n):
    return rng.integers(33, 127, n).astype(np.uint8).tobytes()


def _name(rng, n):
    return _NAME[rng.integers(0, len(_NAME), n)].tobytes()


def case(label, seqs, quals=None, names=None, select=None, base=0, misaligned=False, error=None):
    return dict(label=label, seqs=list(seqs), quals=None if quals is None else list(quals), names=None if names is None else list(names),
                select=None if select is None else [int(bool(x)) for x in select], base=int(base), misaligned=bool(misaligned), error=error)


def _batch(rng, name_lens, base_lens, fastq):
    seqs = [_seq(rng, n) for n in base_lens]
    return dict(seqs=seqs, quals=[_qual(rng, len(s)) for s in seqs] if fastq else None, names=[_name(rng, n) for n in name_lens])


def record_len(name_len, n_bases, fastq):
    return name_len + (2 * n_bases + 6 if fastq else n_bases + 3)


def _fit(total, fastq):
    """(name length, bases) of a record of exactly `total` bytes with a name of 9 .. 11 bytes"""
    for name_len in (10, 9, 11):
        rest = total - name_len - (6 if fastq else 3)
        if rest >= 0 and (not fastq or rest % 2 == 0):
            return name_len, rest // 2 if fastq else rest
    raise AssertionError(total)


def tile_edge_cases():
    out = []
    rng = np.random.default_rng(11)
    for fastq in (False, True):
        tag = "fastq" if fastq else "fasta"
        for end in (TILE - 1, TILE, TILE + 1):             # the first record ends at that byte, and a second follows
            nl, nb = _fit(end, fastq)
            out.append(case(f"end_{end}.{tag}", **_batch(rng, [nl, 7], [nb, 33], fastq)))
    # FASTQ only: a short record, then one whose '\n' '+' '\n' (k = 0, 1, 2) or whose successor's '@' (k = 3) is the first byte of
    # the second tile
    for k in range(4):
        first = record_len(5, 20, True)
        if k < 3:                                          # byte k of \n+\n of record 1 lies at first + 2 + name + len + k
            nl, nb = 8, TILE - k - first - 2 - 8
        else:
            nl, nb = _fit(TILE - first, True)
        out.append(case(f"plus_straddle_{k}.fastq", **_batch(rng, [5, nl, 6], [20, nb, 30], True)))
    return out


def runs_cases():
    rng = np.random.default_rng(12)
    order = [3, 4, 2, 5, 7, 0, 6, 1, 3]                    # (the base runs of the nine records; the 10 000 of the FASTQ batch begins 536 bytes into a tile)
    return [case(f"runs.{'fastq' if fastq else 'fasta'}", **_batch(rng, NAME_RUNS, [BASE_RUNS[i] for i in order], fastq)) for fastq in (False, True)]


def tiny_cases():
    """more units in a tile than lanes in a block: records of 3 and of 6 bytes"""
    return [case("tiny.fasta", [b""] * 1400, None, [b""] * 1400), case("tiny.fastq", [b""] * 700, [b""] * 700, [b""] * 700)]


def select_cases():
    out = []
    rng = np.random.default_rng(13)
    for fastq in (False, True):
        tag = "fastq" if fastq else "fasta"
        n = 40
        b = _batch(rng, rng.integers(0, 30, n), rng.integers(0, 260, n), fastq)
        sel = dict(all=[1] * n, none=[0] * n, first=[1] + [0] * (n - 1), last=[0] * (n - 1) + [1], alternate=[r & 1 for r in range(n)])
        out += [case(f"select_{k}.{tag}", select=v, **b) for k, v in sel.items()]
        n = 5002                                           # two selected records around 5000 unselected ones
        far = _batch(rng, rng.integers(1, 12, n), rng.integers(0, 40, n), fastq)
        out.append(case(f"select_far.{tag}", select=[1] + [0] * 5000 + [1], **far))
        n = 3000                                           # 1 % at random
        sparse = np.zeros(n, np.uint8)
        sparse[rng.choice(n, n // 100, replace=False)] = 1
        out.append(case(f"select_sparse.{tag}", select=sparse.tolist(), **_batch(rng, rng.integers(1, 12, n), rng.integers(0, 40, n), fastq)))
    return out


def generated_name_cases():
    out = []
    rng = np.random.default_rng(14)
    for fastq in (False, True):
        for base in INDEX_BASES:
            b = _batch(rng, [0] * 12, rng.integers(0, 120, 12), fastq)
            out.append(case(f"generated_names_{base}.{'fastq' if fastq else 'fasta'}", b["seqs"], b["quals"], None, [1, 0] * 6 if base == 9 else None, base))
    return out


def misaligned_cases():
    rng = np.random.default_rng(15)
    out = []
    for fastq in (False, True):
        n = 60
        b = _batch(rng, rng.integers(0, 80, n), rng.integers(0, 700, n), fastq)
        out.append(case(f"misaligned.{'fastq' if fastq else 'fasta'}", select=rng.integers(0, 4, n) > 0, misaligned=True, **b))
    return out


def error_cases():
    """each kind alone; the same byte in an unselected record (no error); two offenders (the lowest record wins, then the lowest
    kind); a '\\r' in the middle of a line (written as given)"""
    rng = np.random.default_rng(16)
    out = []
    n = 30

    def fresh(fastq):
        return _batch(rng, rng.integers(3, 30, n), rng.integers(20, 200, n), fastq)

    def spoil(b, what, r, byte=b"\n", at=None):
        v = bytearray(b[what][r])
        v[len(v) // 2 if at is None else at] = byte[0]
        b[what][r] = bytes(v)

    for fastq in (False, True):
        tag = "fastq" if fastq else "fasta"
        for kind, what in ((1, "names"), (2, "seqs"), (3, "quals")):
            if what == "quals" and not fastq:
                continue
            b = fresh(fastq)
            spoil(b, what, 17)
            out.append(case(f"error_kind{kind}.{tag}", error=(17, kind), **b))
            out.append(case(f"error_kind{kind}_unselected.{tag}", select=[r != 17 for r in range(n)], **b))
            b = fresh(fastq)                               # the last byte of the last record, and the first of the first
            spoil(b, what, n - 1, at=-1)
            out.append(case(f"error_kind{kind}_last_byte.{tag}", error=(n - 1, kind), **b))
            b = fresh(fastq)
            spoil(b, what, 0, at=0)
            out.append(case(f"error_kind{kind}_first_byte.{tag}", error=(0, kind), **b))
        b = fresh(fastq)
        spoil(b, "seqs", 9, b"\r")
        spoil(b, "names", 4, b"\r")
        out.append(case(f"carriage_return.{tag}", **b))
        b = fresh(fastq)                                   # the lowest record wins: kind 2 in record 5 against kind 1 in record 6
        spoil(b, "seqs", 5)
        spoil(b, "names", 6)
        out.append(case(f"error_two_records.{tag}", error=(5, 2), **b))
        out.append(case(f"error_two_records_first_unselected.{tag}", select=[r != 5 for r in range(n)], error=(6, 1), **b))
        b = fresh(fastq)                                   # within one record the lowest kind wins
        spoil(b, "seqs", 12)
        spoil(b, "names", 12)
        spoil(b, "names", 20)
        out.append(case(f"error_two_kinds.{tag}", error=(12, 1), **b))
    b = fresh(False)                                       # kind 4: FASTA only; in FASTQ the same bases are fine
    spoil(b, "seqs", 8, b">", at=0)
    out.append(case("error_kind4.fasta", error=(8, 4), **b))
    out.append(case("error_kind4_unselected.fasta", select=[r != 8 for r in range(n)], **b))
    out.append(case("kind4_is_fine.fastq", b["seqs"], [_qual(rng, len(s)) for s in b["seqs"]], b["names"]))
    spoil(b, "seqs", 8)                                    # '>' first and a '\n' behind it: kind 2 is the lower
    out.append(case("error_kind2_and_4.fasta", error=(8, 2), **b))
    b = fresh(False)
    spoil(b, "seqs", 3, b">", at=1)                        # a '>' that is not the first base is a base
    out.append(case("gt_inside.fasta", **b))
    return out


def cases():
    return tile_edge_cases() + runs_cases() + tiny_cases() + select_cases() + generated_name_cases() + misaligned_cases() + error_cases()


def random_case(i):
    rng = np.random.default_rng(1000 + i)
    n = int(rng.integers(0, 48))
    fastq = bool(i & 1)
    base_lens = np.where(rng.random(n) < 0.1, 0, np.where(rng.random(n) < 0.06, rng.integers(2000, 6000, n), rng.integers(1, 160, n)))
    b = _batch(rng, np.where(rng.random(n) < 0.1, 0, rng.integers(1, 70, n)), base_lens, fastq)
    how = int(rng.integers(0, 4))
    select = None if how == 0 else (rng.random(n) < (0.5 if how == 1 else 0.1 if how == 2 else 0.9))
    base = int(rng.choice([0, 7, 95, 10 ** 6 - 3, 2 ** 40]))
    return case(f"random{i}", b["seqs"], b["quals"], b["names"] if i % 3 else None, select, base, misaligned=(i % 5 == 0))


def expected(c):
    """the statement's bytes, or raises ValueError"""
    from sailfish_amd.readfile import reads_text_host
    return reads_text_host(c["seqs"], c["quals"], c["names"], c["select"], c["base"])


def selected(c):
    """[(name, bases, qualities or None)] of the records the text holds"""
    out = []
    for r, s in enumerate(c["seqs"]):
        if c["select"] is None or c["select"][r]:
            out.append((c["names"][r] if c["names"] is not None else b"r%d" % (c["base"] + r), s, None if c["quals"] is None else c["quals"][r]))
    return out


def _odd(a, misaligned):
    """the array as it is handed over: itself, or a copy that starts at an odd byte of its buffer -- at an odd ELEMENT for the
    8-byte offsets, whose typed pointers are aligned to their type: 8 bytes off every 16-byte boundary"""
    if not misaligned:
        return np.ascontiguousarray(a)
    raw = np.zeros(a.nbytes + 48, np.uint8)
    want = 3 if a.itemsize == 1 else 8
    start = (want - raw.ctypes.data) % 16 + 16
    raw[start:start + a.nbytes] = a.view(np.uint8).reshape(-1)
    out = raw[start:start + a.nbytes].view(a.dtype)
    assert out.ctypes.data % 16 == want
    return out


def arrays(c):
    """numpy arrays of a case as the C interface takes them: bases, off (int64), qual, names, name_off (uint64), select -- each
    None where absent, each off its natural 16-byte boundary when the case is misaligned (_odd)"""
    mis = c["misaligned"]
    lens = np.array([len(s) for s in c["seqs"]], np.int64)
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    blob = lambda parts: np.frombuffer(b"".join(parts) or b"\0", np.uint8).copy()
    out = dict(bases=_odd(blob(c["seqs"]), mis), off=_odd(off, mis), qual=None, names=None, name_off=None, select=None, n=len(lens))
    if c["quals"] is not None:
        out["qual"] = _odd(blob(c["quals"]), mis)
    if c["names"] is not None:
        noff = np.zeros(len(lens) + 1, np.uint64)
        np.cumsum([len(x) for x in c["names"]], out=noff[1:])
        out["names"], out["name_off"] = _odd(blob(c["names"]), mis), _odd(noff, mis)
    if c["select"] is not None:
        out["select"] = _odd(np.array(c["select"] or [0], np.uint8), mis)
    return out
