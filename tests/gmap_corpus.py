"""The gene-map files that tests/test_gmap_cpu.py (the serial rules of csrc/gtffmt.h) and tests/test_gpu_gmap.py (the kernels of
csrc/genemap.hip) both read: a corner corpus in each form, seeded random files drawn from its pieces, and the inputs that must be
flagged for the host reader.  Everything is bytes; the expected maps come from genes.TranscriptGeneMap.from_gtf / .from_file."""
import random

KEYS = ("gene_id", "gene_name", "tag", "transcript_id")
NAME_CAP = 256                                         # csrc/gtffmt.h: kGmapNameCap
NAME_LENGTHS = (1, 7, 8, 9, 15, 16, 17, 24, 25, NAME_CAP)


def _name(n, salt="n"):
    """n bytes, distinct per (n, salt)"""
    return (salt + "ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789._-" * 8)[:n]


def gtf_line(attrs, cols=9, pad="", feature="exon", end="\n"):
    c = ["chr1", "SRC" + pad, feature, "100", "200", ".", "+", ".", attrs, 'transcript_id "tenth"; gene_id "tenth";'][:cols]
    return "\t".join(c) + end


# attribute columns; `{t}` / `{g}` are filled in by the random files
PIECES = [
    'gene_id "{g}"; transcript_id "{t}"; gene_name "N{g}"; tag "basic";',
    'transcript_id "{t}"; gene_id "{g}"; gene_name "N{g}"',
    'gene_id "{g}";transcript_id "{t}";tag "x";tag "y";',
    ' gene_id "{g}" ;  transcript_id   "{t}"  ;; ;gene_name "N{g}";;',
    'transcript_id "{t}"; exon_number 3; note "no key here"',
    'gene_id "{g}"; gene_name "N{g}";',                                   # a gene record: no transcript_id
    'transcript_id {t}; gene_id {g}; tag;',
    'transcript_idx "{t}"; my_transcript_id "{t}"; gene_id "{g}";',
    'note "x; transcript_id {t}"; gene_id "{g}"; gene_name "a b  c";',
    'transcript_id "{t}"; gene_id ""; gene_name ";',
    '\x0btranscript_id "{t}"\x0c;\x1cgene_id\x1f"{g}";\x1dgene_name \x1e"N{g}"\x1e',
    'transcript_id "{t}"; gene_id "first{g}"; gene_id "{g}"; transcript_id "other";',
    'transcript_id "{t}"; gene_id',
    'transcript_id; gene_id "{g}"',
    'transcript_id ""; gene_id "{g}";',
    'gene_id   "{g}"; transcript_id "{t}"; tag ""quoted""; gene_name " q "',
]


def corner_gtf():
    L = []
    add = L.append
    add("#!genome-build transcript_id \"comment\"; gene_id \"comment\";\n")
    add("\n"); add("   \n"); add(" \t \x0b\n"); add("\x0c\x1c\x1d\x1e\x1f \n"); add("\t\t\t\t\t\t\t\t\n"); add("\t\t\t\t\t\t\t\t \x0b \n")
    add(gtf_line('transcript_id "eight"; gene_id "eight";', cols=8))
    add("chr1\tS\texon\t1\t2\t.\t+\ttranscript_id \"seven\"; gene_id \"g7\";\n")
    add(gtf_line('transcript_id "nine"; gene_id "g9"; gene_name "n9"; tag "t9";', cols=9))
    add(gtf_line('transcript_id "ten"; gene_id "g10"; gene_name "n10"; tag "t10";', cols=10))
    add(gtf_line('transcript_id "crlf"; gene_id "gcr"; gene_name "ncr"; tag "tcr"', end="\r\n"))
    add(gtf_line('transcript_id "crlf2"; gene_id "gcr";', end="\r\n"))
    add(" #not a comment\tS\texon\t1\t2\t.\t+\t.\ttranscript_id \"sp_hash\"; gene_id \"gsh\";\n")
    for i, p in enumerate(PIECES):
        add(gtf_line(p.format(t=f"piece{i:02d}", g=f"gp{i % 5}"), pad="x" * (i % 16)))
    # the key absent on a transcript's first records and present on a later one; never present; empty first
    for k in range(3):
        add(gtf_line('transcript_id "t_late"; exon_number %d;' % k))
    add(gtf_line('transcript_id "t_late"; gene_id "g_late"; gene_name "n_late"; tag "tag_late";'))
    add(gtf_line('transcript_id "t_late"; gene_id "g_later"; gene_name "n_later"; tag "tag_later";'))
    add(gtf_line('transcript_id "t_never"; exon_number 1;'))
    add(gtf_line('transcript_id "t_never";'))
    add(gtf_line('transcript_id "t_empty_first"; gene_id ""; gene_name ""; tag "";'))
    add(gtf_line('transcript_id "t_empty_first"; gene_id "g_not_me"; gene_name "n_not_me"; tag "x";'))
    # name lengths, names equal in their first 8 and 16 bytes, a name that is a prefix of another
    for n in NAME_LENGTHS:
        add(gtf_line(f'transcript_id "{_name(n, "t")}"; gene_id "{_name(n, "g")}"; gene_name "{_name(n, "m")}"; tag "{_name(n, "u")}";', pad="p" * (n % 16)))
    for tail in ("", "A", "B", "AAAAAAAA", "AAAAAAAAA", "AAAAAAAAB", "AAAAAAAB"):
        t = "SAMEHEAD" + tail
        add(gtf_line(f'transcript_id "{t}"; gene_id "G{t}"; gene_name "SAMEHEADSAMEHEAD{tail}"; tag "{tail}";'))
    for t in ("pre", "prefix", "prefixes", "pref"):
        add(gtf_line(f'gene_id "shared_gene"; transcript_id "{t}"; gene_name "{t}"; tag "shared";'))
    add(gtf_line('transcript_id "z_last"; gene_id "gp0"; gene_name "Ngp0"; tag "basic";'))
    add(gtf_line('transcript_id "no_newline"; gene_id "g_nn"; gene_name "n_nn"; tag "t_nn";', end=""))
    return "".join(L).encode("ascii")


def corner_tsv():
    L = ["t1 g1\n", "t2\tg2\n", "  t3 \x0b g1  \r\n", "\n", "   \n", "t4 g3 t5 g2 t6 g4\n", "t1 g5\n", "t1 g1\n", "dup gA\ndup gB\n",
         "split_over\nlines gS\x0cformfeed\x1cgF\x1dt7\x1eg7\x1ft8 g8\n"]
    for n in NAME_LENGTHS:
        L.append(f"{_name(n, 't')} {_name(n, 'g')}\n")
    for tail in ("", "A", "B", "AAAAAAAA", "AAAAAAAAA", "AAAAAAAAB", "AAAAAAAB"):
        L.append(f"SAMEHEAD{tail}\tSAMEHEADSAMEHEAD{tail}\n")
    for t in ("pre", "prefix", "prefixes", "pref"):
        L.append(f"{t} shared\n")
    L.append("odd_one_out")                                                # an odd token count, no final newline
    return "".join(L).encode("ascii")


def random_gtf(seed, n_lines=2000):
    rng = random.Random(seed)
    n_t, n_g = 150, 40
    tn = [rng.choice(["ENST", "T", "SAMEHEADSAMEHEAD", ""]) + "%0*d" % (rng.choice([1, 4, 8, 11]), rng.randrange(10 ** 4)) + rng.choice(["", ".1", ".12"])
          for _ in range(n_t)]
    gn = [rng.choice(["ENSG", "G", "SAMEHEAD"]) + "%0*d" % (rng.choice([1, 5, 11]), rng.randrange(10 ** 3)) for _ in range(n_g)]
    out = []
    for i in range(n_lines):
        r = rng.random()
        if r < 0.03:
            out.append(rng.choice(["\n", "# comment\n", "  \n", "short\tline\n"]))
            continue
        t = rng.randrange(n_t)
        g = (t * 7 + (rng.randrange(n_g) if rng.random() < 0.05 else 0)) % n_g
        p = PIECES[0] if rng.random() < 0.5 else rng.choice(PIECES)
        out.append(gtf_line(p.format(t=tn[t], g=gn[g]), cols=rng.choice([9, 9, 9, 10, 8]), pad="p" * (i % 16),
                            end=rng.choice(["\n", "\n", "\r\n"])))
    text = "".join(out)
    if seed % 2:
        text = text.rstrip("\r\n")
    return text.encode("ascii")


def random_tsv(seed, n_pairs=2000):
    rng = random.Random(1000 + seed)
    seps = [" ", "\t", "\n", "\r\n", "  ", " \x0b", "\x0c", "\x1c", "\x1f\n"]
    toks = []
    for _ in range(n_pairs):
        toks.append(rng.choice(["T", "SAMEHEAD", "SAMEHEADSAMEHEAD"]) + str(rng.randrange(600)))
        toks.append("G" + str(rng.randrange(80)))
    if seed % 2:
        toks.append("odd")
    return ("".join(t + rng.choice(seps) for t in toks) + ("" if seed % 3 else "\n")).encode("ascii")


# (name, is_gtf, bytes, flag): inputs the device rules do not parse (GT_HOST_* of csrc/gtffmt.h)
HIGH_BYTE, NUL, LONE_CR, LONG_NAME = 1, 2, 4, 8


def flagged():
    ok = gtf_line('transcript_id "a"; gene_id "g";')
    return [
        ("high_gtf", True, (ok + gtf_line('transcript_id "café"; gene_id "g";')).encode("utf-8"), HIGH_BYTE),
        ("high_tsv", False, "a g\nb c d\n".encode("utf-8"), HIGH_BYTE),
        ("nul_gtf", True, (ok + gtf_line('transcript_id "a\0b"; gene_id "g";')).encode("ascii"), NUL),
        ("nul_tsv", False, b"a g\nb\0 c\n", NUL),
        ("cr_gtf", True, (ok.rstrip("\n") + "\r" + ok).encode("ascii"), LONE_CR),
        ("cr_end_gtf", True, (ok + ok.rstrip("\n") + "\r").encode("ascii"), LONE_CR),
        ("cr_tsv", False, b"a g\rb h\n", LONE_CR),
        ("long_tid_gtf", True, (ok + gtf_line(f'transcript_id "{"L" * (NAME_CAP + 1)}"; gene_id "g";')).encode("ascii"), LONG_NAME),
        ("long_gene_gtf", True, (ok + gtf_line(f'transcript_id "b"; gene_id "{"L" * (NAME_CAP + 1)}";')).encode("ascii"), LONG_NAME),
        ("long_tsv", False, ("a g\n" + "L" * (NAME_CAP + 1) + " h\n").encode("ascii"), LONG_NAME),
    ]
