"""CPU tests of the Gibbs sampler's multinomial chain and class visits (sailfish_amd/csrc/gibbsfmt.h compiled as plain C++ by
tests/sampling_harness.cpp -- the header the kernels of gibbs.hip call): the chain against the exact multinomial law, and the harness's
serial restatement of sfgpu_gibbs_sample (gibbs_serial) against the oracle's sequential sampler.  tests/test_gpu_rng.py then holds the
device to the same harness draw for draw and chain for chain; the cases and the plan restated here are shared with it.

gibbs_serial restates the plan with at most kWideSerial = 64 wide classes (phases: light classes, then heavy ones; then the wide
classes in class order).  The coloured and the thin-component orders of the wide classes are not restated: they stay under the z-tests
of tests/test_gpu_configs.py.

Mutants, each applied to gibbsfmt.h in a scratch copy and run once (not committed):
  * `p_rem -= p; if (p_rem < 0.0) p_rem = 0.0;` dropped from multinomial_chain: test_chain_matches_the_multinomial_law fails in five
    of its six cases, every one with a third member -- in (1500, [.5, .3, .2]) a member's mean is 840.0 for 750 against a bound of
    0.4 (the two-member case cannot see it: one binomial).
  * `a.round + 1` -> `a.round` in gibbs_round_class's Philox stream: the law does not depend on which stream a round draws from as long
    as it is its own, so only a trajectory sees it.  Harness built from the mutant against the unmutated harness: every chain of
    test_gpu_rng.py's three problems differs from the first round's sample on (64 of 64, 128 of 128, 70 of 70).  Device library built
    from the mutant against the unmutated harness on an MI355X: test_gibbs_is_the_restatement_chain_by_chain fails in all nine runs,
    every chain differing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_sampling_cpu import _check_against_scipy

HERE = os.path.dirname(os.path.abspath(__file__))
P = C.c_void_p
LIGHT_MAX, WIDE_SPAN, TILE, WIDE_SERIAL = 1500, 2048, 64, 64            # gibbsfmt.h: kGibbsLightMax, kWideSpan, kGibbsTile, kWideSerial

N_DRAWS = 60000
CHAIN_CASES = [(700, [3.0, 1.0]),
               (1500, [.5, .3, .2]),
               (400, [1e-8 / 900, 2.5, 1e-8 / 1200, .7]),                    # prior-only members
               (1400, list(np.random.default_rng(1).random(17) + .01)),
               (3_000_000, [5.0, 1.0, 1e-3, 4.0, 2.0]),
               (200_000, [1e-13, 1e9, 3e8, 1.0])]


def chain_runs():
    """-> [(case, n, weights, last, light)]: `last` at every position for k <= 5, else 0, k / 2, k - 1 and the largest member; the LIGHT form
    (inversion only) next to the other where n <= 1500, as the phase kernels divide the classes"""
    runs = []
    for ci, (n, w) in enumerate(CHAIN_CASES):
        w = np.asarray(w, np.float64); k = len(w)
        lasts = range(k) if k <= 5 else sorted({0, k // 2, k - 1, int(np.argmax(w))})
        for last in lasts:
            for light in ((0, 1) if n <= LIGHT_MAX else (0,)):
                runs.append((ci, n, w, int(last), light))
    return runs


def build_harness(tmp_path_factory, *defs):
    so = tmp_path_factory.mktemp("hc") / "libharness.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", *defs, "-o", str(so), os.path.join(HERE, "sampling_harness.cpp")])
    L = C.CDLL(str(so))
    L.draw_binomial.argtypes = [C.c_uint64, C.c_uint32, C.c_double, C.c_uint32, P]
    L.draw_binomial_by_inversion.argtypes = [C.c_uint64, C.c_uint32, C.c_double, C.c_uint32, P]
    L.draw_uniform_sub.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, P]
    L.draw_words.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, P]
    L.philox_block.argtypes = [C.c_uint32] * 6 + [P]
    L.tree_multinomial.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, P, C.c_uint32, P]
    L.draw_chain.argtypes = [C.c_int, P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, P]
    L.gibbs_serial.argtypes = [C.c_uint64, C.c_uint64, P, P, P, P, P, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, P, C.c_uint32, P]
    L.gibbs_serial.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return build_harness(tmp_path_factory)


def host_chain(H, n, w, last, light, count=N_DRAWS):
    """-> [count, k] draws of the chain, seed 777 + last"""
    w = np.ascontiguousarray(w, np.float64)
    out = np.zeros((count, len(w)), np.uint32)
    H.draw_chain(light, w.ctypes.data, len(w), n, last, 777 + last, count, out.ctypes.data)
    return out


def check_chain_law(x, n, w):
    """x[N, k] draws of Multinomial(n, w / sum w): every draw sums to n; a member of n p < 1e-6 never gets a read; every other member's
    marginal is Binomial(n, p_i) by the three statistics of test_sampling_cpu._check_against_scipy; the covariance of the two largest
    members is -n p_a p_b within 6 standard errors (normal approximation of the product moment: (var_a var_b + cov^2) / N)"""
    N, k = x.shape
    p = w / w.sum()
    assert np.all(x.sum(1, dtype=np.int64) == n)
    for i in range(k):
        if n * p[i] < 1e-6:
            assert not x[:, i].any(), i
            continue
        col = np.ascontiguousarray(x[:, i])
        _check_against_scipy(lambda seed, n_, p_, cnt, ptr: C.memmove(ptr, col.ctypes.data, cnt * 4), n, float(p[i]))
    a, b = np.argsort(p)[-2:]
    xa, xb = x[:, a].astype(np.float64), x[:, b].astype(np.float64)
    cov = np.mean((xa - xa.mean()) * (xb - xb.mean()))
    want = -n * p[a] * p[b]
    se = np.sqrt((n * p[a] * (1 - p[a]) * n * p[b] * (1 - p[b]) + want * want) / N)
    assert abs(cov - want) < 6 * se, (cov, want, se)


@pytest.mark.parametrize("case", range(len(CHAIN_CASES)))
def test_chain_matches_the_multinomial_law(H, case):
    """multinomial_chain on the host, both forms, `last` at every position (chain_runs): check_chain_law over 60000 draws each"""
    for ci, n, w, last, light in chain_runs():
        if ci == case:
            check_chain_law(host_chain(H, n, w, last, light), n, w)


# ---- the plan of sfgpu_gibbs_sample, restated (k_gibbs_plan, gibbs_phase_count) ----
def gibbs_plan(rowptr, ids, counts):
    """-> (kind[C] uint8: 0 light, 1 wide, 2 heavy;  K: the number of phases)"""
    Cn = len(rowptr) - 1
    kind = np.zeros(Cn, np.uint8)
    n_tiles = (Cn + TILE - 1) // TILE
    lo = np.full(n_tiles, 0xFFFFFFFF, np.int64); hi = np.zeros(n_tiles, np.int64)
    for c in range(Cn):
        m = ids[rowptr[c]:rowptr[c + 1]]
        if len(m) == 0:
            continue
        mn, mx = int(m.min()), int(m.max())
        if mx - mn > WIDE_SPAN:
            kind[c] = 1
            continue
        kind[c] = 2 if (len(m) > 1 and counts[c] > LIGHT_MAX) else 0
        t = c // TILE
        lo[t] = min(lo[t], mn); hi[t] = max(hi[t], mx)
    K = 1
    for i in range(n_tiles):
        if lo[i] > hi[i]:
            continue
        d = 1
        while i + d < n_tiles and lo[i + d:].min() <= hi[i]:
            d += 1
        K = max(K, d)
    return kind, K


def host_gibbs(H, eff, mass, rowptr, ids, counts, R, n_chains, seed, rounds, kind, K):
    """-> [rounds * n_chains, M] int32, the samples sfgpu_gibbs_sample emits"""
    eff = np.ascontiguousarray(eff, np.float64); mass = np.ascontiguousarray(mass, np.float64)
    rp = np.ascontiguousarray(rowptr, np.uint32); ii = np.ascontiguousarray(ids, np.uint32); cc = np.ascontiguousarray(counts, np.uint64)
    kind = np.ascontiguousarray(kind, np.uint8)
    out = np.zeros((rounds * n_chains, len(eff)), np.int32)
    rc = H.gibbs_serial(len(eff), len(rp) - 1, rp.ctypes.data, (ii if len(ii) else np.zeros(1, np.uint32)).ctypes.data, cc.ctypes.data,
                        eff.ctypes.data, mass.ctypes.data, int(R), n_chains, seed, rounds * n_chains, kind.ctypes.data, K, out.ctypes.data)
    assert rc == 0
    return out


def test_restatement_matches_the_sequential_sampler(H, built):
    """gibbs_serial against the oracle's sequential sampleRound_ (src/CollapsedGibbsSampler.cpp:113-184) with the statistics of
    test_gpu_configs.test_gibbs_multi_phase_round_matches_the_sequential_sampler: a multi-phase plan (K >= 2) with three wide classes
    and heavy classes among the light ones, 256 chains of 40 rounds against 64 oracle chains -- the restatement is a Gibbs sampler of
    the reference's law before the device is held to it chain by chain"""
    from oracle import oracle as O
    from sailfish_amd import synth
    M, Pn, R = 3000, 6000, 60_000
    ref_len, ids, off = synth.workload(M, Pn, R)
    ids = ids.numpy().view(np.uint32); off = off.numpy().view(np.uint32).astype(np.uint64)
    rng = np.random.default_rng(5)
    wide = [np.sort(rng.choice(M, 6, replace=False)).astype(np.uint32) for _ in range(3)]
    reps = 400
    n0 = int(off[20])                                              # the first 20 reads 2000 times more: heavy classes
    ids = np.concatenate([ids, np.tile(ids[:n0], 2000)] + [np.tile(w, reps) for w in wide])
    lens = np.concatenate([np.diff(off), np.tile(np.diff(off[:21]), 2000)] + [np.full(reps, len(w), np.uint64) for w in wide])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    R = len(off) - 1
    ob = O.EqBuilder(); ob.add_batch(ids, off)
    rp, ii, cc, _ = ob.finish()
    eff = O.efflen_smoothed(ref_len.numpy().view(np.uint32), O.cf_gaussian())
    rc, _, mass, _ = O.em_optimize(eff, rp, ii, cc, R)
    assert rc == 0
    kind, K = gibbs_plan(rp.astype(np.int64), ii, cc)
    assert K >= 2 and (kind == 1).sum() >= 3 and (kind == 2).sum() >= 1 and (kind == 0).sum() > 1000
    n_chains, rounds, burn = 256, 40, 12
    g = host_gibbs(H, eff, mass, rp, ii, cc, R, n_chains, 21, rounds, kind, K).reshape(rounds, n_chains, M)
    assert np.all(g.sum(2) == R)
    gm = g[burn:].mean(0)
    n_oc = 64
    om = []
    for c in range(n_oc):
        orc, og = O.gibbs(eff, mass, rp.astype(np.uint64), ii, cc, R, rounds, seed=1000 + c)
        assert orc == 0 and np.all(og.sum(1) == R)
        om.append(og[burn:].mean(0))
    om = np.stack(om)
    mg, mo = gm.mean(0), om.mean(0)
    vg, vo = gm.var(0, ddof=1), om.var(0, ddof=1)
    fixed = (vg == 0) & (vo == 0)
    assert fixed.sum() > 0 and np.array_equal(mg[fixed], mo[fixed])
    z = (mg - mo) / np.sqrt(vg / n_chains + vo / n_oc + 0.02)
    assert float(np.mean(np.abs(z) > 4.0)) < 0.01 and float(np.max(np.abs(z))) < 8.0, (np.sort(np.abs(z))[-10:],)
    assert abs(float(np.mean(z))) < 0.15
    mv = vo > 9.0
    assert mv.sum() > 50
    ratio = np.sqrt(vg[mv] / vo[mv])
    assert 0.8 < float(np.median(ratio)) < 1.25 and float(np.mean((ratio > 0.5) & (ratio < 2.0))) > 0.95
    wt = np.unique(np.concatenate(wide))
    assert float(np.max(np.abs(z[wt]))) < 6.0


def test_harness_is_clean_under_sanitizers(tmp_path):
    """the chain, the class visits and gibbs_serial in a stand-alone program (tests/gibbs_sanitize_main.cpp: its own main, nothing
    loaded into Python) built with -fsanitize=address,undefined: an empty class, a singleton, a heavy and a wide class, a last
    round that emits only some of the chains"""
    exe = tmp_path / "gibbs_sanitize"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           os.path.join(HERE, "gibbs_sanitize_main.cpp")])
    r = subprocess.run([str(exe)], text=True, capture_output=True)
    assert r.returncode == 0 and "sanitize ok" in r.stdout, r.stdout + r.stderr
