"""CPU tests of the VBEM x arithmetic (sailfish_amd/csrc/vbmath.h compiled as plain C++ by tests/vbmath_harness.cpp, -ffp-contract=off)
against tests/golden/vbmath_vectors.npz: mpmath at 60 digits, rounded once to binary64 (tests/golden/make_vbmath_vectors.py).
tests/test_gpu_vbmath.py holds the device forms to the same file under the same bounds.

The bound follows the shape of the error instead of one flat tolerance (which would have to admit the worst point -- alpha at the
prior, an exponent of -128 -- and hide a wrong high-order coefficient where it would show, at y in [10, 12] with a small exponent):

    x forms     |got - want| / want  <=  K  2^-53 (1 + |psi(a) - c| + r(a))        r(a) = sum_{k<10} 1 / (a + k) below 10, else 0
    psi         |got - want|         <=  K0 2^-53 (max(1, |psi|) + r(x))

K and K0 are MEASURED: the smallest values with which the host forms pass over the committed grid, times 2 (the margin is for
libm's exp / log against the device's).  Measured over the grid (g++ 13, glibc): exp(digamma_pos - c) / len 13.76, vb_x_lean 15.48,
vb_x_fast 15.48, digamma_pos 3.12.  The worst x point is a = 1.8e9, c = 21.3: psi(a) and c cancel to -0.04 there, so the half ulp
of each (21 x 2^-53) is 15 times what the shape allows a small exponent; over [10, 12] with c = psi(a + 1) the forms measure 3 - 5.

The bound can fail.  Each mutant below was applied by hand to a scratch copy of the header (all host forms that hold the constant)
and test_host_forms_against_mpmath run on it; the figure is the K (K0) the mutant needs, against the 31 (6.25) it is given:

    mutant                                              x forms 1 / 2 / 3                 psi          verdict
    series 1/120 -> 1/252                               3.6e9                             1.7e9        caught
    series 1/252 -> 1/240                               1.6e6                             7.9e5        caught
    series 1/240 -> 1/252                               1.6e4  (rel 2.0e-12)              7.9e3        caught
    series 1/132 -> 1/240                               2.8e3  (rel 3.4e-13)              1.4e3        caught
    series B12 691/32760 -> 1/12                        5.1e2  (rel 6.2e-14)              2.5e2        caught
    series B14 1/12 -> 1/13                             unchanged                         unchanged    NOT seen: 6e-17 at y = 10, below an ulp
    ln2_lo -> 0            (vb_x_fast only)             - / - / 5.7e7 (rel 7.4e-9)        -            caught
    Taylor 1/24 -> 1/25    (vb_x_fast only)             - / - / 2.8e11                    -            caught
    Taylor r^13 term -> 0  (vb_x_fast only)             unchanged                         -            NOT seen: |r|^13 / 13! <= 1.7e-16
    recurrence of 9 terms (the shift stays 10)          2.8e14                            2.9e14       caught

So everything through B12 and the whole exp except its last term is pinned; B14 and r^13 lie below the rounding of binary64 at the
arguments the forms can see (y >= 10, |r| <= ln 2 / 2) and no test in binary64 can see them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
VECTORS = os.path.join(GOLD, "vbmath_vectors.npz")

K_X = 31.0          # 2 x 15.48 (rounded up), the measured K of vb_x_lean and vb_x_fast; exp(digamma_pos - c) / len measures 13.76
K_PSI = 6.25        # 2 x 3.12 (rounded up), the measured K0 of digamma_pos
ULP_HALF = 2.0 ** -53


def r_of(a):
    """sum_{k<10} 1 / (a + k) where the recurrence runs (a < 10), else 0"""
    a = np.asarray(a, np.float64)
    with np.errstate(divide="ignore", over="ignore"):
        return np.where(a < 10.0, (1.0 / (a[:, None] + np.arange(10.0))).sum(1), 0.0)


def x_scale(z):
    """2^-53 (1 + |psi(a) - c| + r(a)) per point of the x grid; psi(a) - c = log(want len), to 1e-16 of itself"""
    return ULP_HALF * (1.0 + np.abs(np.log(z["x_want"] * z["x_len"])) + r_of(z["x_a"]))


def psi_scale(z):
    fin = np.isfinite(z["psi_want"])
    with np.errstate(over="ignore"):
        return np.where(fin, ULP_HALF * (np.maximum(1.0, np.abs(z["psi_want"])) + r_of(z["psi_x"])), 0.0)


def x_excess(got, z):
    """max over the x grid of |got - want| / want in units of the scale (to compare with a K), and the point"""
    k = np.abs(got - z["x_want"]) / z["x_want"] / x_scale(z)
    k = np.where(np.isfinite(k), k, np.inf)
    i = int(np.argmax(k))
    return float(k[i]), i


def psi_excess(got, z):
    """the same for the psi grid; where psi overflows binary64 the value must be -inf itself"""
    fin = np.isfinite(z["psi_want"])
    assert np.array_equal(got[~fin], z["psi_want"][~fin]), (z["psi_x"][~fin], got[~fin])
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(fin, np.abs(got - z["psi_want"]) / np.where(fin, psi_scale(z), 1.0), 0.0)
    k = np.where(np.isfinite(k), k, np.inf)
    i = int(np.argmax(k))
    return float(k[i]), i


def load_vectors():
    with np.load(VECTORS) as f:
        return {k: f[k] for k in f.files}


def build_harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("vb") / "libvbmath.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), os.path.join(HERE, "vbmath_harness.cpp")])
    L = C.CDLL(str(so))
    L.vb_eval_host.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.vb_eval_host.restype = C.c_int
    return L


def host_eval(L, form, a, c=None, length=None):
    a = np.ascontiguousarray(a, np.float64)
    c = a if c is None else np.ascontiguousarray(c, np.float64)
    length = a if length is None else np.ascontiguousarray(length, np.float64)
    out = np.full(len(a), np.nan)
    assert L.vb_eval_host(form, a.ctypes.data, c.ctypes.data, length.ctypes.data, len(a), out.ctypes.data) == 0
    return out


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return build_harness(tmp_path_factory)


@pytest.fixture(scope="module")
def Z():
    return load_vectors()


def test_fixture_covers_the_edges(Z):
    """what the grid has to hold for the bounds to mean anything (a regenerated file keeps it)"""
    a, ln, px = Z["x_a"], Z["x_len"], Z["psi_x"]
    for v in (0.01, 0.01 + 2.0 ** -40, 0.01 + 1, 0.01 + 20, np.nextafter(10.0, 0.0), 10.0, np.nextafter(10.0, np.inf)):
        assert (a == v).any(), v
    for v in (1.0, np.nextafter(1.0, 2.0), 1e6):
        assert (ln == v).any(), v
    near = (a >= 10.0) & (a <= 12.0) & (ln == 1.0) & (np.abs(np.log(Z["x_want"])) < 0.2)
    assert near.sum() >= 300 and a.min() == 0.01 and a.max() > 2.0 ** 39 and Z["x_c"].max() < 50.0 and ln.min() == 1.0
    for v in (np.finfo(np.float64).smallest_subnormal, 1e-310, 1e-300, 1e-100, 1e-8, 1e-3, 2.0 ** 60):
        assert (px == v).any(), v
    assert np.isneginf(Z["psi_want"][px <= 1e-309]).all() and np.isfinite(Z["psi_want"][px >= 1e-308]).all()
    assert 2000 <= len(a) <= 5000 and os.path.getsize(VECTORS) <= 150151          # no larger than the other .npz fixtures


def test_fixture_is_what_mpmath_gives(Z):
    """the committed expectations, recomputed: every psi and x expectation of a stride through the grids (all of the special points),
    the toys' and the random problem's loops -- bit for bit"""
    pytest.importorskip("mpmath")
    sys.path.insert(0, GOLD)
    import make_vbmath_vectors as G
    sel = np.r_[0:312, 312:len(Z["x_a"]):9]
    np.testing.assert_array_equal(G.expect_x(Z["x_a"][sel], Z["x_c"][sel], Z["x_len"][sel]), Z["x_want"][sel])
    sel = np.r_[0:40, 40:len(Z["psi_x"]):9]
    np.testing.assert_array_equal(G.psi_double(Z["psi_x"][sel]), Z["psi_want"][sel])
    probs = G.problems()
    assert tuple(probs) == G.PROBLEMS
    for name, prob in probs.items():
        for key, val in zip(("eff", "rp", "ii", "cc"), prob):
            np.testing.assert_array_equal(Z[f"p_{name}_{key}"], val)
        assert int(Z[f"p_{name}_N"]) == prob[4]
        for vb in (False, True):
            for n in G.LOOP_ITERS if name != "lowdepth" else (1,):
                np.testing.assert_array_equal(G.loop_expectation(prob, vb, n), Z[f"p_{name}_{'vb' if vb else 'em'}_{n}"])


@pytest.mark.parametrize("form,name", [(1, "exp(digamma_pos - c) / len"), (2, "vb_x_lean"), (3, "vb_x_fast")])
def test_host_forms_against_mpmath(H, Z, form, name):
    got = host_eval(H, form, Z["x_a"], Z["x_c"], Z["x_len"])
    k, i = x_excess(got, Z)
    print(f"{name}: measured K = {k:.3f} at a = {Z['x_a'][i]!r}, c = {Z['x_c'][i]!r}, len = {Z['x_len'][i]!r}")
    assert k <= K_X, (name, k, Z["x_a"][i], Z["x_c"][i], Z["x_len"][i], got[i], Z["x_want"][i])


def test_host_digamma_against_mpmath(H, Z):
    got = host_eval(H, 0, Z["psi_x"])
    k, i = psi_excess(got, Z)
    print(f"digamma_pos: measured K0 = {k:.3f} at x = {Z['psi_x'][i]!r}")
    assert k <= K_PSI, (k, Z["psi_x"][i], got[i], Z["psi_want"][i])


def test_host_forms_agree_pairwise(H, Z):
    """two forms that each lie within the bound of the truth lie within twice the bound of each other"""
    g = {f: host_eval(H, f, Z["x_a"], Z["x_c"], Z["x_len"]) for f in (1, 2, 3)}
    for f1, f2 in ((1, 2), (1, 3), (2, 3)):
        assert (np.abs(g[f1] - g[f2]) <= 2.0 * K_X * x_scale(Z) * Z["x_want"]).all(), (f1, f2)


def test_where_the_domain_ends(H):
    """The x forms are defined for a >= the prior (0.01), len >= 1, c < 50.  Below it the forms with an exp of their own break: at a = 1e-100 the
    argument is -1e100, which rint / ldexp do not reduce, and vb_x_fast returns -inf (-0.0 at a = 1e-30) -- no finite positive
    number -- while libm's exp gives the other two forms the true answer, an x that underflows to 0.  Nothing inside vb_x_fast /
    vb_x_head guards this: it is the CALLERS' guarantee -- new_alpha adds the prior to every alpha' before an x is formed from it
    (alpha' >= prior), and the first x of a run, whose alpha N / n_active may lie below the prior, comes from digamma_pos
    (k_vb_prepare) -- that keeps it out of a sweep, and the reason that guarantee matters."""
    a, c, ln = np.array([1e-100]), np.array([3.0]), np.array([100.0])
    bad = host_eval(H, 3, a, c, ln)[0]
    assert not (np.isfinite(bad) and bad > 0.0), bad
    assert host_eval(H, 1, a, c, ln)[0] == 0.0 and host_eval(H, 2, a, c, ln)[0] == 0.0      # exp(-1e100) = 0: the true x underflows
    # ... and at the prior itself, with the largest normaliser and length of the domain, all three are finite, positive and agree
    a, c, ln = np.array([0.01]), np.array([49.0]), np.array([3e5])
    g = [host_eval(H, f, a, c, ln)[0] for f in (1, 2, 3)]
    assert all(np.isfinite(v) and v > 0.0 for v in g) and max(g) / min(g) - 1.0 < 1e-12, g
