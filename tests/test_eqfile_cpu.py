"""CPU tests of the class-file reader's host side (sailfish_amd/eqfile.py, quant.fld_counts_for_requant): the header (M, C,
names), the refusals that name a file line, the numpy writer against the writer's loop, and the FLD-branch rule of requantify."""
import numpy as np
import pytest


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_bytes(text.encode() if isinstance(text, str) else text)
    return str(p)


def _loop_writer(names, rowptr, ids, counts):
    """writer.write_equiv_counts' loop, restated over plain arrays (GZipWriter.cpp:51-92)"""
    s = f"{len(names)}\n{len(counts)}\n" + "".join(n + "\n" for n in names)
    for c in range(len(counts)):
        lab = ids[rowptr[c]:rowptr[c + 1]]
        s += f"{len(lab)}\t" + "".join(f"{t}\t" for t in lab) + f"{counts[c]}\n"
    return s.encode()


def test_header_is_parsed(built, tmp_path):
    from sailfish_amd import eqfile
    p = _write(tmp_path, "a.txt", "3\n2\ntx0\ntx1\ntx2\n1\t0\t5\n2\t2\t1\t7\n")
    h = eqfile.read_header(p)
    assert (h.n_transcripts, h.n_classes, h.names, h.header_lines) == (3, 2, ["tx0", "tx1", "tx2"], 5)
    assert open(p, "rb").read()[h.data_offset:] == b"1\t0\t5\n2\t2\t1\t7\n"
    eqfile.check_names(h, ["tx0", "tx1", "tx2"])
    # a table without classes ends with the names
    h = eqfile.read_header(_write(tmp_path, "b.txt", "1\n0\nx\n"))
    assert (h.n_classes, h.names) == (0, ["x"])


@pytest.mark.parametrize("text, line, what", [
    ("3x\n1\na\nb\nc\n", 1, "decimal integer"),
    ("3\n-1\na\nb\nc\n", 2, "decimal integer"),
    (" 3\n1\na\nb\nc\n", 1, "decimal integer"),
    ("3\r\n1\r\na\r\n", 1, "decimal integer"),
    ("", 1, "empty file"),
    ("3", 1, "ends inside the header"),
    ("3\n1\na\nb", 4, "ends after 1 of the M=3"),            # truncated names
    ("4\n1\na\nb\nc\n1\t0\t5\n", 6, "transcript name 4 of M=4"),   # M larger than the names: a class line where a name belongs
])
def test_header_refusals_name_the_line(built, tmp_path, text, line, what):
    from sailfish_amd import eqfile
    p = _write(tmp_path, "bad.txt", text)
    with pytest.raises(ValueError) as e:
        eqfile.read_header(p)
    assert f"{p}, line {line}:" in str(e.value) and what in str(e.value), str(e.value)


def test_wrong_m_and_names_are_refused(built, tmp_path):
    from sailfish_amd import eqfile
    p = _write(tmp_path, "a.txt", "3\n0\ntx0\ntx1\ntx2\n")
    h = eqfile.read_header(p)
    with pytest.raises(ValueError, match=r"line 1: the header lists M=3 transcripts, expected 4"):
        eqfile.check_names(h, ["tx0", "tx1", "tx2", "tx3"])
    with pytest.raises(ValueError, match=r"line 4: transcript 1 is named 'tx1', expected 'tY'"):
        eqfile.check_names(h, ["tx0", "tY", "tx2"])


def test_lanes_must_list_the_same_names(built, tmp_path):
    from sailfish_amd import eqfile
    a = eqfile.read_header(_write(tmp_path, "a.txt", "3\n0\ntx0\ntx1\ntx2\n"))
    b = eqfile.read_header(_write(tmp_path, "b.txt", "3\n0\ntx0\ntx2\ntx1\n"))
    c = eqfile.read_header(_write(tmp_path, "c.txt", "2\n0\ntx0\ntx1\n"))
    eqfile.check_same_names([a, a])
    with pytest.raises(ValueError) as e:
        eqfile.check_same_names([a, b])
    assert f"{b.path}, line 4: transcript 1 is named 'tx2', expected 'tx1'" in str(e.value)
    with pytest.raises(ValueError) as e:
        eqfile.check_same_names([a, c])
    assert f"{c.path}, line 1:" in str(e.value) and "M=2" in str(e.value)


def test_numpy_writer_matches_the_loop(built):
    from sailfish_amd import eqfile
    rng = np.random.default_rng(5)
    C = 500
    k = rng.integers(1, 30, C)
    rowptr = np.zeros(C + 1, np.int64); rowptr[1:] = np.cumsum(k)
    ids = rng.integers(0, 10 ** 6, int(rowptr[-1])).astype(np.uint32)
    counts = rng.integers(0, 2 ** 63, C, dtype=np.uint64) >> rng.integers(0, 63, C).astype(np.uint64)
    counts[:3] = [0, 2 ** 64 - 1, 10 ** 19]
    names = [f"t{i}" for i in range(7)]
    assert eqfile.format_text(names, rowptr, ids, counts) == _loop_writer(names, rowptr, ids, counts)
    assert eqfile.format_text(names, [0], [], []) == _loop_writer(names, [0], [], [])


def test_fld_branch_rule(built):
    """requantify takes the prior exactly when the stored counts are getNormalFragLengthCounts' element for element"""
    import sailfish_amd as sf
    sopt = sf.SailfishOpts()
    prior = sf.efflen.normal_counts(sopt)
    assert sf.quant.fld_counts_for_requant(prior.copy(), sopt) is None
    emp = prior.copy(); emp[250] += 1
    got = sf.quant.fld_counts_for_requant(emp, sopt)
    assert got is not None and got.dtype == np.uint32 and np.array_equal(got, emp)
    # other prior parameters give other counts: the same file read with them is the empirical branch
    assert sf.quant.fld_counts_for_requant(prior, sf.SailfishOpts(fragLenDistPriorMean=250)) is not None
    zeros = np.zeros(sopt.maxFragLen, np.int32)        # noEffectiveLengthCorrection runs store zeros
    assert np.array_equal(sf.quant.fld_counts_for_requant(zeros, sopt), zeros)
