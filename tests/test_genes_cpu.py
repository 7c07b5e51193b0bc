"""The host/device headers of the gene-level path compiled as plain C++ with g++ (tests/genes_harness.cpp), and the vectorised
name lookup.  No GPU.
  * gfmt_value (sailfish_amd/csrc/gfmt.h): the double strtod reads back from a printed %g token, by bit pattern;
  * gene_fold (sailfish_amd/csrc/genefold.h): one gene of aggregateEstimatesToGeneLevel, against
    genes.aggregate_estimates_to_gene_level by bit pattern (its fmt_g is replaced by one that prints the bits);
  * TranscriptGeneMap.gene_names_of / gene_ids_of against gene_name, one name at a time."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_harness(tmp_path):
    exe = tmp_path / "genes_harness"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "sailfish_amd", "csrc"), os.path.join(ROOT, "tests", "genes_harness.cpp"), "-o", str(exe)])
    return exe


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def harness_fold(exe, tmp_path, gene_of_row, length, eff, tpm, num_reads, printed=False):
    """genefold.h over the table, rows in the order given: [(gene, len bits, eff bits, tpm bits, num_reads bits)] in
    first-appearance order of the genes"""
    table = tmp_path / "fold_table.txt"
    with open(table, "w") as f:
        for i in range(len(gene_of_row)):
            f.write(f"{int(gene_of_row[i])} {int(length[i])} {bits(eff[i]):016x} {bits(tpm[i]):016x} {bits(num_reads[i]):016x}\n")
    r = subprocess.run([str(exe), "fold", str(table)] + (["printed"] if printed else []), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return [(int(w[0]),) + tuple(int(x, 16) for x in w[1:]) for w in (line.split() for line in r.stdout.splitlines())]


def test_gfmt_value_matches_strtod(tmp_path):
    exe = build_harness(tmp_path)
    r = subprocess.run([str(exe), "value", "1000000"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    s = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w and w[0] == "set":
            s[w[1]] = dict(checked=int(w[3]), failures=int(w[5]), slow=int(w[7]), cross=int(w[9]))
        elif w and w[0] == "ties":
            s["n_ties"] = int(w[1])
    assert set(s) == {"random_bits", "columns", "ties", "decades", "denormals", "edges", "n_ties"}, r.stdout
    for name in ("random_bits", "columns", "ties", "decades", "denormals", "edges"):
        assert s[name]["failures"] == 0, r.stdout
    assert s["columns"]["checked"] >= 1_000_000 and s["random_bits"]["checked"] >= 250_000
    assert s["n_ties"] >= 40_000 and s["ties"]["checked"] == 4 * s["n_ties"]
    assert s["decades"]["checked"] >= 629 * 3 + 628 * 4 and s["denormals"]["checked"] >= 200_000
    # no quant-like value (tokens between 1e-16 and 1e9) leaves the one-operation window; the multi-word half is exercised, and
    # was compared with the fast half on a sample of the values both answer
    assert s["columns"]["slow"] == 0 and s["ties"]["slow"] == 0, r.stdout
    assert s["random_bits"]["slow"] > 0 and s["decades"]["slow"] > 0 and s["edges"]["slow"] > 0, r.stdout
    assert s["denormals"]["slow"] == s["denormals"]["checked"]
    assert s["columns"]["cross"] > 10_000


def random_table(rng, sizes, n_filler):
    """columns of a quant.sf whose genes have the given sizes (and n_filler genes of random small sizes), rows of a gene
    interleaved with the others'; about a third of the genes unexpressed.  Returns (gene_of_row, length, eff, tpm, num_reads)
    with gene numbers 0 .. G-1 in no particular row order"""
    sizes = list(sizes) + [int(x) for x in rng.integers(1, 9, n_filler)]
    gene = np.repeat(np.arange(len(sizes)), sizes)
    n = len(gene)
    length = rng.integers(200, 100_000, n).astype(np.uint32)
    eff = np.maximum(length.astype(np.float64) - rng.random(n) * 180.0, 1.0)
    cnt = np.where(rng.random(n) < 0.2, 0.0, 10.0 ** rng.uniform(-6, 5, n))
    unexpressed = rng.random(len(sizes)) < 1 / 3
    cnt[unexpressed[gene]] = 0.0
    rate = cnt / eff
    tpm = rate / rate.sum() * 1e6 if rate.sum() > 0 else np.zeros(n)
    perm = rng.permutation(n)
    return gene[perm], length[perm], eff[perm], tpm[perm], cnt[perm], unexpressed


def host_bits(monkeypatch, tmp_path, names, gene_names, length, eff, tpm, num_reads):
    """genes.aggregate_estimates_to_gene_level on the quant.sf of these columns, with its fmt_g printing bit patterns:
    [(gene name, len bits, eff bits, tpm bits, num_reads bits)] in file order"""
    from sailfish_amd import genes
    tgm = genes.TranscriptGeneMap(list(zip(names, gene_names)))
    q = tmp_path / "quant.sf"
    with open(q, "w") as f:
        f.write("Name\tLength\tEffectiveLength\tTPM\tNumReads\n")
        for i, nm in enumerate(names):
            f.write("%s\t%d\t%s\t%s\t%s\n" % (nm, int(length[i]), "%g" % eff[i], "%g" % tpm[i], "%g" % num_reads[i]))
    monkeypatch.setattr(genes, "fmt_g", lambda x: "%016x" % bits(x))
    out = genes.aggregate_estimates_to_gene_level(tgm, str(q))
    monkeypatch.undo()
    rows = [line.split("\t") for line in open(out).read().split("\n")[1:] if line]
    return [(r[0],) + tuple(int(x, 16) for x in r[1:]) for r in rows]


def printed(a):
    return np.array([float("%g" % x) for x in a])


@pytest.mark.parametrize("seed", [11, 12])
def test_gene_fold_matches_the_host_loop(tmp_path, monkeypatch, seed):
    rng = np.random.default_rng(seed)
    gene, length, eff, tpm, cnt, unexpressed = random_table(rng, [1, 2, 3, 64, 65, 300, 300, 65, 64, 3, 2, 1], 700)
    # two more genes: one whose totalTPM IS denorm_min (a single row: the comparison is strict, it takes the 1 / n branch) and
    # one whose totalTPM is a larger denormal (5e-324 + (5e-324 + 5e-324): the weighted branch, weights 1/3 and 1/3)
    G = int(gene.max()) + 1
    gene = np.concatenate([gene, [G, G + 1, G + 1]])
    length = np.concatenate([length, [1000, 700, 300]]).astype(np.uint32)
    eff = np.concatenate([eff, [800.0, 650.5, 120.25]])
    tpm = np.concatenate([tpm, [5e-324, 5e-324, 5e-324]])
    cnt = np.concatenate([cnt, [1.0, 2.0, 3.0]])
    n = len(gene)
    assert 3000 <= n <= 6000 and 0.2 < unexpressed.mean() < 0.45
    names = [f"t{i:05d}" for i in range(n)]
    gene_names = [f"g{g}" for g in gene]
    want = host_bits(monkeypatch, tmp_path, names, gene_names, length, eff, tpm, cnt)
    exe = build_harness(tmp_path)
    # the printed values, rounded here by Python and, second, by gfmt_decode -> gfmt_value inside the harness
    got = harness_fold(exe, tmp_path, gene, length, printed(eff), printed(tpm), printed(cnt))
    got2 = harness_fold(exe, tmp_path, gene, length, eff, tpm, cnt, printed=True)
    assert len(got) == len(want) == G + 2
    for g, g2, w in zip(got, got2, want):
        assert (f"g{g[0]}",) + g[1:] == w
        assert g2 == g
    by_name = {w[0]: w for w in want}
    assert by_name[f"g{G}"][1:3] == (bits(1000.0), bits(800.0))
    third = printed([5e-324])[0] / (3 * 5e-324)
    assert by_name[f"g{G + 1}"][1] == bits(0.0 + 700 * third + 300 * third)
    # the running-sum quirk is pinned: the same fold with totalTPM = sum(tpm) gives other lengths on this table
    p_tpm = printed(tpm)
    differs = 0
    for g in range(G):
        rows = np.flatnonzero(gene == g)
        total = 0.0
        for r in rows:
            total += p_tpm[r]
        if not total > 5e-324:
            continue
        gl = 0.0
        for r in rows:
            gl += float(length[r]) * (p_tpm[r] / total)
        differs += bits(gl) != by_name[f"g{g}"][1]
    assert differs > 100


def _tgm(transcripts, gene_names, t2g):
    from sailfish_amd import genes
    tgm = genes.TranscriptGeneMap.__new__(genes.TranscriptGeneMap)
    tgm.transcript_names, tgm.gene_names, tgm.t2g = list(transcripts), list(gene_names), list(t2g)
    return tgm


def _check_lookup(tgm, queries):
    want = [tgm.gene_name(q) for q in queries]
    assert tgm.gene_names_of(queries) == want
    ids, table = tgm.gene_ids_of(queries)
    assert ids.dtype == np.uint32 and [table[i] for i in ids] == want
    # gene identity is the name: equal names, equal ids, and the other way round
    seen = {}
    for i, w in zip(ids.tolist(), want):
        assert seen.setdefault(w, i) == i
    assert len(set(seen.values())) == len(seen)
    assert table[:len(tgm.gene_names)] == tgm.gene_names


def test_gene_names_of_matches_gene_name():
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_tgm_vectors.json")))["cases"]
    n = 0
    for case in cases:
        tgm = _tgm(case["transcripts"], case["genes"], case["t2g"])
        assert tgm.gene_names_of(case["queries"]) == case["gene_of_query"]
        _check_lookup(tgm, case["queries"])
        n += len(case["queries"])
    assert n > 300
    from sailfish_amd import genes
    rng = np.random.default_rng(5)
    alphabet = ["a", "b", "ab", "t", "T", "0", "9", "_", ".", "|", "é", "ß", "к", "転", "😀", "~"]
    for trial in range(30):
        def word():
            return "".join(rng.choice(alphabet, int(rng.integers(1, 7))))
        base = sorted({word() for _ in range(int(rng.integers(1, 60)))})
        # names that are prefixes of one another
        base = sorted(set(base + [b + "x" for b in base[::3]] + [b[:-1] for b in base[::4] if len(b) > 1]))
        pairs = [(t, f"G{int(rng.integers(0, max(2, len(base) // 3)))}") for t in base]
        if trial % 5 == 0:
            pairs.append((base[0] + "own", "G0"))
        tgm = genes.TranscriptGeneMap([pairs[i] for i in rng.permutation(len(pairs))])
        queries = [t for t, _ in pairs] + [word() for _ in range(80)]                   # present and (mostly) absent names
        queries += ["~~~~" + word() for _ in range(10)] + ["\U0010ffff", "~~~~dup", "~~~~dup"]      # past the end: their own genes
        queries += ["G0", "G1", "zzzzG", tgm.gene_names[0]]                               # own-gene names that may collide with a map gene
        queries += [q + "x" for q in queries[:10]] + [q[:-1] for q in queries[:10] if len(q) > 1]
        _check_lookup(tgm, [queries[i] for i in rng.permutation(len(queries))])
    # a map gene named like a transcript beyond the last name: that transcript joins the gene
    tgm = genes.TranscriptGeneMap([("tA", "zz"), ("tB", "g2")])
    ids, table = tgm.gene_ids_of(["tA", "zz", "zy", "zz"])
    assert ids.tolist() == [0, 0, 2, 0] and table == ["zz", "g2", "zy"]              # no entry for the own name that joined
    empty = genes.TranscriptGeneMap([])
    assert empty.gene_names_of(["b", "a"]) == ["b", "a"] and empty.gene_names_of([]) == []
    _check_lookup(empty, ["b", "a", "b"])
