"""Quantify from saved class files (sailfish_amd/eqfile.py, sfgpu_eq_add_text_host, quant.quantify_eq_classes / requantify,
loadEquivClasses in include/sfgpu_sailfish.hpp): the device parse against insertGroups, chunk edges, the round trip through a
finished run's output, merging lanes, malformed input, and the C++ adaptor."""
import gzip
import os
import subprocess

import numpy as np
import pytest
import torch

from test_filter import _txome

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(eq):
    return eq.eqVec().to_numpy()


def _assert_same_table(a, b):
    for x, y, what in zip(a, b, ("rowptr", "ids", "counts", "hashes")):
        assert x.dtype == y.dtype and np.array_equal(x, y), what


def _reference_table(classes, M, gpu):
    """the table insertGroups builds from the same classes"""
    import sailfish_amd as sf
    rowptr, ids, counts = classes
    eq = sf.EquivalenceClassBuilder(device=gpu)
    eq.start()
    eq.insertGroups(torch.from_numpy(ids.astype(np.uint32).view(np.int32)).to(gpu),
                    torch.from_numpy(rowptr.astype(np.uint32).view(np.int32)).to(gpu),
                    torch.from_numpy(counts.astype(np.uint64).view(np.int64)).to(gpu))
    eq.finish()
    return _table(eq)


def _random_classes(rng, C, M, long_label=0):
    k = rng.integers(1, 13, C)
    wide = rng.random(C) < 0.01
    k[wide] = rng.integers(1, 301, int(wide.sum()))
    if long_label:
        k[C // 2] = long_label
    rowptr = np.zeros(C + 1, np.int64); rowptr[1:] = np.cumsum(k)
    ids = rng.integers(0, M, int(rowptr[-1])).astype(np.uint32)            # ordered as written, repeats allowed
    counts = rng.integers(1, 1000, C).astype(np.uint64)
    big = rng.random(C) < 0.05
    counts[big] = rng.integers(2 ** 32, 2 ** 40, int(big.sum()), dtype=np.uint64)
    # a few labels written twice (lanes of one run): the fold adds their counts
    dup = rng.choice(C, 1000, replace=False)
    lab = [ids[rowptr[c]:rowptr[c + 1]] for c in dup]
    k2 = np.concatenate([k, [len(x) for x in lab]])
    rowptr2 = np.zeros(len(k2) + 1, np.int64); rowptr2[1:] = np.cumsum(k2)
    return rowptr2, np.concatenate([ids] + lab), np.concatenate([counts, rng.integers(1, 50, len(dup)).astype(np.uint64)])


def _fold(path, names, gpu, chunk_bytes=0):
    import sailfish_amd as sf
    eq = sf.EquivalenceClassBuilder(device=gpu)
    eq.start()
    res = eq.add_eq_file(path, names=names, chunk_bytes=chunk_bytes)
    eq.finish()
    return eq, res


@pytest.mark.gpu
def test_parse_parity_at_scale(built, gpu, tmp_path):
    """>= 1 M classes, >= 8 M ids, labels of 1 .. 300 ids, one of 100 000, counts above 2^32: the parsed table is the
    insertGroups table bit for bit"""
    from sailfish_amd import eqfile
    rng = np.random.default_rng(11)
    M = 200_000
    classes = _random_classes(rng, 1_050_000, M, long_label=100_000)
    rowptr, ids, counts = classes
    assert len(counts) >= 1_000_000 and len(ids) >= 8_000_000
    names = [f"ENST{i:08d}" for i in range(M)]
    p = tmp_path / "eq.txt"
    p.write_bytes(eqfile.format_text(names, rowptr, ids, counts))
    eq, res = _fold(str(p), names, gpu)
    assert res["n_lines"] == len(counts) and res["n_ids"] == len(ids) and res["n_chunks"] >= 2
    assert res["sum_counts"] == int(counts.sum(dtype=np.uint64))
    assert eq.total_reads == int(counts.sum(dtype=np.uint64))
    _assert_same_table(_table(eq), _reference_table(classes, M, gpu))


@pytest.mark.gpu
def test_chunk_edges(built, gpu, tmp_path):
    """a few-KB chunk: lines straddle every chunk boundary; a label as long as a chunk still parses; one longer is refused"""
    from sailfish_amd import _lib, eqfile
    rng = np.random.default_rng(12)
    M = 5000
    rowptr, ids, counts = _random_classes(rng, 20_000, M, long_label=700)     # ~3.5 KB line
    names = [f"t{i}" for i in range(M)]
    p = tmp_path / "eq.txt"
    p.write_bytes(eqfile.format_text(names, rowptr, ids, counts))
    want = _reference_table((rowptr, ids, counts), M, gpu)
    for chunk in (4096, 4099, 1 << 16):
        eq, res = _fold(str(p), names, gpu, chunk_bytes=chunk)
        assert res["n_chunks"] > 1
        _assert_same_table(_table(eq), want)
    with pytest.raises(ValueError) as e:
        _fold(str(p), names, gpu, chunk_bytes=2048)
    assert "longer than the chunk size" in str(e.value) and f"line {2 + M + 20_000 // 2 + 1}:" in str(e.value), str(e.value)
    # the first class line is the long one: refused before anything is staged
    q = tmp_path / "first.txt"
    q.write_bytes(eqfile.format_text(names, np.array([0, 700]), ids[:700], counts[:1]))
    with pytest.raises(ValueError) as e:
        _fold(str(q), names, gpu, chunk_bytes=2048)
    assert "longer than the chunk size" in str(e.value) and f"line {2 + M + 1}:" in str(e.value), str(e.value)
    # a builder that has been finished refuses the fold of the first chunk, while the second is on its way to the device
    with pytest.raises(_lib.SfgpuError) as e:
        eq.add_eq_file(str(p), names=names, chunk_bytes=4096)
    assert e.value.code == _lib.ERR_STATE


def _hit_batches(rng, rl, R, paired, n_batches=3):
    from oracle import oracle as O
    M = len(rl)
    out = []
    for _ in range(n_batches):
        n = R // n_batches
        j = rng.integers(0, M // 2, n)
        shared = rng.random(n) < 0.9
        k = np.where(shared, 2, 1)
        off = np.zeros(n + 1, np.uint32); off[1:] = np.cumsum(k)
        h = np.zeros(int(off[-1]), O.HIT_DTYPE)
        first = off[:-1].astype(np.int64)
        h["tid"][first] = 2 * j
        h["tid"][first[shared] + 1] = 2 * j[shared] + 1
        L = rl[h["tid"]].astype(np.int64)
        h["frag_len"] = rng.integers(120, 260, len(h))
        left = (rng.random(len(h)) * np.maximum(L - 260, 1)).astype(np.int32)
        fw = np.repeat(rng.integers(0, 2, n), k)
        h["read_len"] = 50; h["fwd"] = fw
        if paired:
            h["mate_status"] = 3
            h["pos"] = np.where(fw == 1, left, left + h["frag_len"] - 50); h["mate_pos"] = np.where(fw == 1, left + h["frag_len"] - 50, left)
            h["mate_len"] = 50; h["mate_fwd"] = 1 - fw
        else:
            h["mate_status"] = 0
            h["pos"] = left
        out.append((h, off))
    return out


def _quant_cols(path):
    rows = [l.split("\t") for l in open(path).read().strip().split("\n")]
    return [r[:3] for r in rows]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["single_em", "single_vbem", "paired_em", "paired_vbem", "paired_bias"])
def test_round_trip_through_the_output(built, gpu, tmp_path, case):
    """quantify(dumpEq) -> requantify(output dir): same table, effective lengths, stop iteration, estimates, quant.sf columns
    and bootstraps"""
    import sailfish_amd as sf
    rng = np.random.default_rng(21)
    M, R = 400, 90_000
    seq, so, rl = _txome(rng, M, lo=400, hi=3000)
    names = [f"tx{i:04d}" for i in range(M)]
    paired = case.startswith("paired")
    kw = dict(useVBOpt=case.endswith("vbem"), biasCorrect=case.endswith("bias"), numFragSamples=2000, numBootstraps=3)
    batches = _hit_batches(rng, rl, R, paired)
    out1, out2 = str(tmp_path / "run1"), str(tmp_path / "run2")
    rc, e1 = sf.quant.quantify(names, rl, batches, "IU" if paired else "U", out1, sf.SailfishOpts(dumpEq=True, **kw), seq=seq, seq_off=so,
                               allow_orphans=True, num_bias_samples=5000, seed=7, device=gpu)
    assert rc == 0
    fld = np.frombuffer(gzip.open(os.path.join(out1, "aux", "fld.gz")).read(), np.int32)
    took_prior = sf.quant.fld_counts_for_requant(fld, sf.SailfishOpts(**kw)) is None
    assert took_prior == (not paired)                      # single end: the prior; paired with enough pairs: the counts
    extra = dict(seq=seq, seq_off=so, num_fwd=e1.numFwd(), num_rc=e1.numRC()) if kw["biasCorrect"] else {}
    rc, e2 = sf.quant.requantify(out1, out2, sf.SailfishOpts(**kw), seed=7, device=gpu, **extra)
    assert rc == 0
    _assert_same_table(_table(e1.equivalenceClassBuilder()), _table(e2.equivalenceClassBuilder()))
    assert e2.numMappedFragments() == e1.numMappedFragments()
    t1, t2 = e1.transcripts(), e2.transcripts()
    rel = lambda x, y: float(np.max(np.abs(x - y) / np.maximum(np.abs(x), 1e-300)))
    l1, l2 = t1.EffectiveLength.cpu().numpy(), t2.EffectiveLength.cpu().numpy()
    s1, s2 = e1.last_optimizer_stats, e2.last_optimizer_stats
    a, b = t1.estCount.cpu().numpy(), t2.estCount.cpu().numpy()
    if kw["biasCorrect"]:
        # the bias recompute sums its expected k-mer weights with double atomics (bias.hip): two runs of quantify itself differ in
        # the last bits of the bias-corrected lengths, so this case is held to a tolerance
        assert rel(l1, l2) <= 1e-9 and rel(a, b) <= 1e-9, (rel(l1, l2), rel(a, b))
    else:
        assert np.array_equal(l1, l2)
        assert s1["iters"] == s2["iters"]
        if s1["persistent"] == s2["persistent"]:
            assert np.array_equal(a, b)
        else:
            assert rel(a, b) <= 1e-12
    assert _quant_cols(os.path.join(out1, "quant.sf")) == _quant_cols(os.path.join(out2, "quant.sf"))
    bs = [np.frombuffer(gzip.open(os.path.join(o, "aux", "bootstrap", "bootstraps.gz")).read(), np.float64) for o in (out1, out2)]
    assert bs[0].size == 3 * M
    assert np.max(np.abs(bs[0] - bs[1]) / np.maximum(np.abs(bs[0]), 1.0)) <= (1e-7 if kw["biasCorrect"] else 1e-9)


@pytest.mark.gpu
def test_lanes_merge(built, gpu, tmp_path):
    """the files of two disjoint halves of the reads fold into the table one builder over all reads gives"""
    import sailfish_amd as sf
    from sailfish_amd import eqfile, synth
    M, P, R = 3000, 8000, 300_000
    ref_len, ids, off = synth.workload(M, P, R, device="cpu")
    ids, off = ids.numpy().view(np.uint32), off.numpy().view(np.uint32)
    names = [f"t{i}" for i in range(M)]
    sopt = sf.SailfishOpts()
    paths = []
    for h, (r0, r1) in enumerate(((0, R // 2), (R // 2, R))):
        exp = sf.ReadExperiment(sf.Transcripts(names, ref_len.numpy().view(np.uint32), device=gpu), sopt)
        eq = exp.equivalenceClassBuilder(); eq.start()
        eq.add_batch(ids[off[r0]:off[r1]], off[r0:r1 + 1] - off[r0]); eq.finish()
        d = str(tmp_path / f"lane{h}")
        sf.writer.write_equiv_counts(d, exp, sopt)
        paths.append(os.path.join(d, "aux", "eq_classes.txt"))
        rp, ii, cc, _ = _table(eq)                              # the numpy writer writes the writer's bytes
        assert eqfile.format_text(names, rp, ii, cc) == open(paths[-1], "rb").read()
    whole = sf.EquivalenceClassBuilder(device=gpu); whole.start(); whole.add_batch(ids, off); whole.finish()
    merged = sf.EquivalenceClassBuilder(device=gpu); merged.start()
    _, results = eqfile.fold_files(merged, paths, names=names)
    merged.finish()
    assert sum(r["n_lines"] for r in results) > merged.n_classes      # classes seen in both lanes were added up
    assert merged.total_reads == whole.total_reads
    _assert_same_table(_table(merged), _table(whole))
    # lanes must list the same names
    bad = tmp_path / "bad.txt"
    bad.write_bytes(open(paths[1], "rb").read().replace(b"\nt7\n", b"\nt7x\n", 1))
    with pytest.raises(ValueError, match=r"bad.txt, line 10: transcript 7 is named 't7x', expected 't7'"):
        eqfile.fold_files(sf.EquivalenceClassBuilder(device=gpu), [paths[0], str(bad)])


def _small_file(M=50, C=300, seed=3):
    from sailfish_amd import eqfile
    rng = np.random.default_rng(seed)
    k = rng.integers(1, 6, C)
    rowptr = np.zeros(C + 1, np.int64); rowptr[1:] = np.cumsum(k)
    ids = rng.integers(0, M, int(rowptr[-1]))
    counts = rng.integers(1, 100, C).astype(np.uint64)
    names = [f"n{i}" for i in range(M)]
    return names, (rowptr, ids, counts), eqfile.format_text(names, rowptr, ids, counts)


def _replace_class_line(text, M, i, new):
    lines = text.split(b"\n")
    lines[2 + M + i] = new
    return b"\n".join(lines)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [0, 64])
def test_malformed_input_names_the_line(built, gpu, tmp_path, chunk):
    names, classes, text = _small_file()
    M, C = len(names), len(classes[2])
    i = 217                                                       # the class line that is broken (0-based)
    line = 2 + M + i + 1                                          # ... as a 1-based line of the file
    cases = {
        "non_digit": _replace_class_line(text, M, i, b"2\t1x\t3\t5"),
        "k_too_large": _replace_class_line(text, M, i, b"3\t1\t2\t5"),
        "k_too_small": _replace_class_line(text, M, i, b"1\t1\t2\t5"),
        "k_zero": _replace_class_line(text, M, i, b"0\t5"),
        "id_range": _replace_class_line(text, M, i, b"2\t1\t%d\t5" % M),
        "count_overflow": _replace_class_line(text, M, i, b"1\t1\t18446744073709551616"),
        "empty_line": _replace_class_line(text, M, i, b""),
        "empty_field": _replace_class_line(text, M, i, b"2\t1\t\t5"),
        "trailing_tab": _replace_class_line(text, M, i, b"1\t1\t5\t"),
        "space": _replace_class_line(text, M, i, b"1\t1 \t5"),
        "crlf": b"\n".join(l + b"\r" if j >= 2 + M + i and l else l for j, l in enumerate(text.split(b"\n"))),
    }
    expected = {"non_digit": "not a digit", "k_too_large": "label length", "k_too_small": "label length", "k_zero": "label length",
                "id_range": "transcript id", "count_overflow": "64 bits", "empty_line": "empty", "empty_field": "empty",
                "trailing_tab": "empty", "space": "not a digit", "crlf": "CRLF"}
    for what, body in cases.items():
        p = tmp_path / f"{what}.txt"
        p.write_bytes(body)
        with pytest.raises(ValueError) as e:
            _fold(str(p), names, gpu, chunk_bytes=chunk)
        assert f"{p}, line {line}:" in str(e.value) and expected[what] in str(e.value), (what, str(e.value))
    # the header's C against the lines present: the first missing / the first extra class line
    for c_hdr, at in ((C + 1, 2 + M + C + 1), (C - 1, 2 + M + C)):
        p = tmp_path / f"c{c_hdr}.txt"
        p.write_bytes(text.replace(b"\n%d\n" % C, b"\n%d\n" % c_hdr, 1))
        with pytest.raises(ValueError) as e:
            _fold(str(p), names, gpu, chunk_bytes=chunk)
        assert f"line {at}: the header announces C={c_hdr}" in str(e.value), str(e.value)
    # a missing final newline is accepted
    p = tmp_path / "no_final_newline.txt"
    p.write_bytes(text[:-1])
    eq, res = _fold(str(p), names, gpu, chunk_bytes=chunk)
    assert res["n_lines"] == C
    _assert_same_table(_table(eq), _reference_table(classes, M, gpu))


@pytest.mark.gpu
def test_cpp_adaptor_load_equiv_classes(built, gpu, tmp_path):
    """loadEquivClasses in include/sfgpu_sailfish.hpp, compiled with g++ and run: the table equals Python's"""
    names, classes, text = _small_file(M=300, C=20_000, seed=9)
    p = tmp_path / "eq.txt"; p.write_bytes(text)
    (tmp_path / "names.txt").write_text("".join(n + "\n" for n in names))
    bad = tmp_path / "bad.txt"; bad.write_bytes(_replace_class_line(text, len(names), 5, b"2\t1\t999999\t4"))
    exe = tmp_path / "eqfile_host_test"
    csrc = os.path.join(ROOT, "sailfish_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "eqfile_host_test.cpp"), "-o", str(exe),
                           "-L", csrc, "-lsfgpu", "-L", "/opt/rocm/lib", "-lamdhip64", "-pthread",
                           "-Wl,-rpath," + csrc + ",-rpath,/opt/rocm/lib"])
    outb = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(p), str(tmp_path / "names.txt"), str(outb), str(bad)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"bad.txt, line {2 + len(names) + 5 + 1}:" in r.stdout, r.stdout
    raw = outb.read_bytes()
    C, nnz, mapped, observed = np.frombuffer(raw[:32], np.uint64)
    o = 32
    rp = np.frombuffer(raw[o:o + 4 * (C + 1)], np.uint32); o += 4 * (int(C) + 1)
    ii = np.frombuffer(raw[o:o + 4 * nnz], np.uint32); o += 4 * int(nnz)
    cc = np.frombuffer(raw[o:o + 8 * C], np.uint64); o += 8 * int(C)
    hh = np.frombuffer(raw[o:o + 8 * C], np.uint64)
    eq, _ = _fold(str(p), names, gpu)
    _assert_same_table((rp, ii, cc, hh), _table(eq))
    total = int(classes[2].sum())
    assert mapped == observed == total
