"""Writes tests/golden/vbmath_vectors.npz: what tests/test_vbmath_cpu.py and tests/test_gpu_vbmath.py hold the VBEM x arithmetic
(sailfish_amd/csrc/vbmath.h) to.  Every expectation is computed with mpmath at 60 digits from the binary64 INPUTS as stored and
rounded once to binary64 (half an ulp: far below every bound the tests use), so the tests need neither mpmath nor scipy.

  x_a, x_c, x_len          the x grid (forms 1 - 4: exp(psi(a) - c) / len)
  x_want                   the correctly rounded x
  psi_x, psi_want          the psi grid (form 0): the x grid's a and a quarter of its S, x from denorm_min up (-inf where -1/x overflows), up to 2^60
  p_<name>_{eff,rp,ii,cc,N}    four small EM problems;   p_<name>_{em,vb}_{1,2,7}: em_numpy_restatement.optimize_mp after 1, 2, 7 rounds

Run:  python tests/golden/make_vbmath_vectors.py      (needs mpmath; a few seconds)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "vbmath_vectors.npz")
DIGITS = 60
LOOP_ITERS = (1, 2, 7)
PROBLEMS = ("toy5", "toy7", "rand", "lowdepth")


def _mp():
    import mpmath as mp
    mp.mp.dps = DIGITS
    return mp


def _to_double(v):
    """an mpf rounded once to binary64 (nearest even; +-inf beyond the range)"""
    mp = _mp()
    if abs(v) >= mp.mpf(2) ** 1024:
        return -np.inf if v < 0 else np.inf
    return float(v)


def psi_double(x):
    """psi of binary64 values, correctly rounded"""
    mp = _mp()
    return np.array([_to_double(mp.digamma(mp.mpf(float(v)))) for v in x], np.float64)


def expect_x(a, c, length):
    """-> exp(psi(a) - c) / len, correctly rounded, from the binary64 a, c, len"""
    mp = _mp()
    return np.array([_to_double(mp.exp(mp.digamma(mp.mpf(float(ai))) - mp.mpf(float(ci))) / mp.mpf(float(li)))
                     for ai, ci, li in zip(a, c, length)], np.float64)


def x_grid():
    """-> a, S, len of the x grid (c = psi(S) is made by the caller)"""
    rng = np.random.default_rng(20240917)
    lu = lambda lo, hi, n: np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    a, S, ln = [], [], []
    # a transcript's alpha is the prior plus counts; the branch at 10 -- each crossed with the edge lengths and three normalisers
    special = [0.01, 0.01 + 2.0 ** -40] + [0.01 + k for k in range(21)] + [np.nextafter(10.0, 0.0), 10.0, np.nextafter(10.0, np.inf)]
    for av in special:
        for lv in (1.0, np.nextafter(1.0, 2.0), 1e6, 1234.5):
            for sv in (1.01, 5e4, 2.0 ** 40):
                a.append(av); ln.append(lv); S.append(sv)
    # [10, 12] with c = psi(a + 1) and len = 1: no recurrence, an exponent of -1/a -- the floor is a few ulp, the series' higher terms show
    near = np.concatenate([np.linspace(10.0, 12.0, 150), rng.uniform(10.0, 12.0, 150)])
    a += list(near); S += list(near + 1.0); ln += [1.0] * len(near)
    # the bulk: log-uniform a (denser below 20), len and S
    for lo, hi, n in ((0.01, 20.0, 800), (0.01, 2.0 ** 40, 600)):
        a += list(lu(lo, hi, n)); S += list(lu(1.01, 2.0 ** 40, n)); ln += list(lu(1.0, 3e5, n))
    return np.array(a, np.float64), np.array(S, np.float64), np.array(ln, np.float64)


def psi_grid(x_a, x_S):
    rng = np.random.default_rng(20240918)
    # (-1/x overflows below 2^-1024 = 5.6e-309; no point within a few ulp of that edge, where the rounding of the fraction decides)
    tiny = [np.finfo(np.float64).smallest_subnormal, 1e-310, 1e-309, 1e-308, 1e-300, 1e-100, 1e-8, 1e-3]
    wide = np.exp(rng.uniform(np.log(1e-12), np.log(2.0 ** 60), 400))
    return np.unique(np.concatenate([x_a, x_S[::4], tiny, wide, [2.0 ** 60]]))


def problems():
    """name -> (eff, rowptr, ids, counts, num_mapped): the two survey toys, the random 25 x 60 problem of
    test_em_independent.test_oracle_and_numpy_agree_with_mpmath_on_small_problems (same seed, same draws), and a low-depth problem
    whose initial alpha N / n_active = 3 / 700 lies BELOW the prior: the first x of a VBEM run must come from the full digamma_pos"""
    k = json.load(open(os.path.join(HERE, "survey_kat.json")))
    out = {}
    for name in ("em_toy5", "em_toy7"):
        t = k[name]
        eff = np.array(t["ref_len"], float) - t["eff_len_minus"]
        rp = np.zeros(len(t["classes"]) + 1, np.uint64); rp[1:] = np.cumsum([len(c) for c in t["classes"]])
        ii = np.array([x for c in t["classes"] for x in c], np.uint32)
        out[name[3:]] = (eff, rp, ii, np.array(t["counts"], np.uint64), int(t["num_mapped"]))
    rng = np.random.default_rng(11)
    M, C = 25, 60
    lens = rng.integers(1, 7, C)
    rp = np.zeros(C + 1, np.uint64); rp[1:] = np.cumsum(lens)
    ii = np.concatenate([np.sort(rng.choice(M - 3, l, replace=False)) for l in lens]).astype(np.uint32)
    cc = rng.integers(1, 500, C).astype(np.uint64)
    eff = np.concatenate([rng.uniform(0.2, 3.0, 5), rng.uniform(50, 5000, M - 5)])
    out["rand"] = (eff, rp, ii, cc, int(cc.sum()))
    rng = np.random.default_rng(12)
    C, K, step = 3, 300, 200                                  # three single-read classes of 300 members, neighbours share 100
    rp = (np.arange(C + 1) * K).astype(np.uint64)
    ii = np.concatenate([np.arange(c * step, c * step + K) for c in range(C)]).astype(np.uint32)
    out["lowdepth"] = (rng.uniform(200.0, 3000.0, (C - 1) * step + K), rp, ii, np.ones(C, np.uint64), C)
    return out


def loop_expectation(prob, vb, n_iter):
    sys.path.insert(0, os.path.dirname(HERE))
    import em_numpy_restatement as R
    eff, rp, ii, cc, N = prob
    return R.optimize_mp(eff, np.asarray(rp, np.int64), ii, cc, N, vb=vb, n_iter=n_iter, digits=DIGITS)


def main():
    d = {}
    a, S, ln = x_grid()
    c = psi_double(S)
    want = expect_x(a, c, ln)
    d.update(x_a=a, x_c=c, x_len=ln, x_want=want)
    px = psi_grid(a, S)
    d.update(psi_x=px, psi_want=psi_double(px))
    for name, prob in problems().items():
        eff, rp, ii, cc, N = prob
        d.update({f"p_{name}_eff": eff, f"p_{name}_rp": rp, f"p_{name}_ii": ii, f"p_{name}_cc": cc, f"p_{name}_N": np.array(N, np.uint64)})
        for vb in (False, True):
            for n in LOOP_ITERS:
                d[f"p_{name}_{'vb' if vb else 'em'}_{n}"] = loop_expectation(prob, vb, n)
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes;", len(a), "x points,", len(px), "psi points")


if __name__ == "__main__":
    main()
