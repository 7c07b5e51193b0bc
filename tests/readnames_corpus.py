"""Texts and name lists for the read-name tests (tests/test_readnames_cpu.py, tests/test_gpu_readnames.py): what the name blob of
sfgpu_reads_parse_*_n and the mate-name rule (sailfish_amd/csrc/readfmt.h) have to get right.  No test in here."""
import numpy as np

LENS = [0, 1, 15, 16, 17, 31, 33, 48, 49, 300, 5000]
# in this order the 16-byte groups of the blob begin at the start of names (offsets 16, 64, 80, 96, 144), inside them, and names
# end where a group ends; empty names lie at a group boundary and inside a group
ORDER = [16, 48, 0, 1, 15, 16, 17, 31, 33, 48, 49, 300, 5000, 0, 0, 1, 33, 15, 16]
STYLES = ("alone", "space", "tab", "mixed")


def name_bytes(rng, ln):
    """a name of ln bytes: anything printable but the blank and the tab"""
    return rng.integers(33, 127, ln, dtype=np.uint8).tobytes()


def header(name, style, r):
    style = STYLES[r % 3] if style == "mixed" else style
    return name + {"alone": b"", "space": b" extra words", "tab": b"\tx y"}[style]


def render(fmt, names, rng, style="mixed", crlf=False, final_newline=True, empty_records=False):
    """the names as a FASTQ ('@') or FASTA ('>') text; FASTA with empty_records: every third record has no sequence line"""
    eol = b"\r\n" if crlf else b"\n"
    out = []
    for r, nm in enumerate(names):
        ln = int(rng.integers(0, 25))
        seq = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), ln))
        if fmt == "fastq":
            out += [b"@" + header(nm, style, r), seq, b"+", bytes(rng.integers(33, 127, ln, dtype=np.uint8))]
        else:
            out.append(b">" + header(nm, style, r))
            if not (empty_records and r % 3 == 0):
                out += [seq[a:a + 10] for a in range(0, ln, 10)]
    text = eol.join(out) + eol if out else b""
    return text if final_newline or not text else text[:-len(eol)]


def names_with_total(rng, total):
    lens = ORDER[:12] + [17, 31]
    lens = lens + [total - sum(lens)]
    assert lens[-1] > 0
    return [name_bytes(rng, ln) for ln in lens]


def gather_cases():
    """-> (label, text, names) for the whole final text"""
    rng = np.random.default_rng(101)
    base = [name_bytes(rng, ln) for ln in ORDER]
    for fmt in ("fastq", "fasta"):
        for style in STYLES:
            yield f"{fmt}_{style}", render(fmt, base, rng, style), base
            yield f"{fmt}_{style}_crlf", render(fmt, base, rng, style, crlf=True), base
        for total in (4095, 4096, 4097):
            nms = names_with_total(rng, total)
            yield f"{fmt}_total_{total}", render(fmt, nms, rng), nms
    yield "fastq_no_final_newline", render("fastq", base, rng, final_newline=False), base
    yield "fastq_crlf_no_final_newline", render("fastq", base, rng, "alone", crlf=True, final_newline=False), base
    yield "fasta_empty_records", render("fasta", base, rng, empty_records=True), base
    last = base + [name_bytes(rng, 21)]                      # the last record is its header line alone, without a newline
    yield "fasta_header_only_last_line", render("fasta", base, rng, empty_records=True) + b">" + last[-1], last
    yield "fasta_header_only_last_line_crlf", render("fasta", base, rng, "alone", crlf=True) + b">" + last[-1], last


def blob_of(names):
    return b"".join(names), np.concatenate([[0], np.cumsum([len(n) for n in names], dtype=np.int64)]).astype(np.int64)


def match_cases():
    """-> (label, names 1, names 2): lists of equal length; the expected answer comes from readfile.mate_stem"""
    rng = np.random.default_rng(202)
    eq = [name_bytes(rng, ln) for ln in LENS]
    yield "none", [], []
    for ln, nm in zip(LENS, eq):
        yield f"one_equal_{ln}", [nm], [nm]
    yield "equal_all_lengths", eq, list(eq)
    for ln, nm in zip(LENS, eq):
        if ln:
            first = bytes([nm[0] ^ 1]) + nm[1:]
            last = nm[:-1] + bytes([nm[-1] ^ 1])
            yield f"first_byte_{ln}", eq[:3] + [nm], eq[:3] + [first]
            yield f"last_byte_{ln}", eq[:3] + [nm], eq[:3] + [last]
        yield f"length_only_{ln}", eq[:2] + [nm], eq[:2] + [nm + b"x"]
        yield f"suffixes_{ln}", [nm + b"/1", nm + b"/1", nm, nm + b"/2"], [nm + b"/2", nm, nm + b"/2", nm + b"/2"]
    yield "a_1_a_2_a", [b"a/1", b"a/1", b"a", b"a/2", b"a/1"], [b"a/2", b"a", b"a/1", b"a/2", b"a/1"]
    yield "a_3_is_not_a", [b"a/1", b"a/3"], [b"a/2", b"a"]
    yield "a_3_both", [b"a/3"], [b"a/3"]
    yield "slash_1_is_empty", [b"/1", b"", b"/2"], [b"", b"/2", b"/1"]
    yield "slash_alone", [b"/", b"1", b"x/"], [b"/", b"1", b"x/"]
    yield "slash_vs_empty", [b"/"], [b""]
    two = [b"read%d/1" % i for i in range(200)]
    yield "200_equal", two, [n[:-1] + b"2" for n in two]
    bad = [n[:-1] + b"2" for n in two]
    bad[130] = b"read131/2"; bad[3] = b"reaD3/2"
    yield "200_bad_at_130_and_3", two, bad
    bad = [n[:-1] + b"2" for n in two]
    bad[130] = b"read13/2"
    yield "200_bad_at_130", two, bad
    long1 = [name_bytes(rng, 5000) for _ in range(70)]       # several long names in one wavefront, one of them differing deep inside
    long2 = list(long1)
    long2[66] = long1[66][:4321] + bytes([long1[66][4321] ^ 2]) + long1[66][4322:]
    yield "long_names_equal", long1, list(long1)
    yield "long_names_bad_at_66", long1, long2
