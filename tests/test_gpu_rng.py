"""GPU tests (-m gpu) of the samplers on the device: csrc/rng.h (Philox4x32-10, uniform, ratio_of, binv, binomial, binomial_by_inversion),
multinomial_chain and the Gibbs class visits of csrc/gibbsfmt.h, and the multinomial tree of csrc/sampling.hip, through the diagnostic
entries sfgpu_rng_eval, sfgpu_chain_eval and sfgpu_mn_tree_eval and through sfgpu_gibbs_sample -- against the exact laws
(test_sampling_cpu._check_against_scipy, imported) and, draw for draw, against the host build of the same headers
(tests/sampling_harness.cpp).  Every draw is a function of (seed, stream, substream, arguments), so device and host may differ only
where their arithmetic does: ratio_of (reciprocal plus two Newton steps for the division) and ocml for glibc's exp / log1p / log.

The caps on differing draws (1e-4 of the draws; one vector; one chain) are conditions, not tolerances: on the host a ratio_of off by
one ulp, and a build with contraction and the native instruction set, each changed 0 of 1 740 000 binomial draws.  Host against host
every figure below is 0.  The Gibbs restatement covers the plan with at most kWideSerial wide classes (test_chain_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import test_chain_cpu as T
import test_sampling_cpu as S
from test_sampling_cpu import _check_against_scipy

pytestmark = pytest.mark.gpu

WORDS, UNIFORM, RATIO, BINOMIAL, BINOMIAL_INV, BLOCK = range(6)          # include/sfgpu.h: SFGPU_RNG_*
SENTINEL = 0xDEADBEEF
BINV_MAX_MEAN = 110.0                                                    # rng.h: kBinvMaxMean


def _params(fn):
    return [tuple(a) for m in fn.pytestmark if m.name == "parametrize" for a in m.args[1]]


BINOMIAL_CASES = _params(S.test_binomial_matches_scipy)                 # the (n, p) of the host's tests, not copies of them
INVERSION_CASES = _params(S.test_binomial_by_inversion_matches_scipy)
EDGE_CASES = [(0, 0.5), (77, 0.0), (77, 1.0)]                           # test_binomial_edges
assert len(BINOMIAL_CASES) == 29 and len(INVERSION_CASES) == 14


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return T.build_harness(tmp_path_factory)


def _u64(gpu, v):
    import torch
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, np.uint64).view(np.int64)).to(gpu)


def rng_eval(gpu, form, seed, n, stream=None, sub=None, cnt=None, a=None, b=None, w=0, guard=0):
    """-> (rc, out as numpy, [n (* w) + guard]; SENTINEL / NaN where the kernel did not write)"""
    import torch
    from sailfish_amd import _lib
    f64 = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, np.float64)).to(gpu)
    ts, tb, ta, tbb = _u64(gpu, stream), _u64(gpu, sub), f64(a), f64(b)
    tn = None if cnt is None else torch.from_numpy(np.ascontiguousarray(cnt, np.uint32).view(np.int32)).to(gpu)
    per = w if form in (WORDS, UNIFORM) else (4 if form == BLOCK else 1)
    if form not in (UNIFORM, RATIO):
        out = torch.full((n * per + guard,), SENTINEL - (1 << 32), dtype=torch.int32, device=gpu)
    else:
        out = torch.full((n * per + guard,), float("nan"), dtype=torch.float64, device=gpu)
    rc = _lib.lib().sfgpu_rng_eval(form, seed, _lib.ptr(ts), _lib.ptr(tb), _lib.ptr(tn), _lib.ptr(ta), _lib.ptr(tbb), w, n, _lib.ptr(out),
                                   _lib.current_stream_ptr())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return rc, (o.view(np.uint32) if o.dtype == np.int32 else o)


def draw_device(gpu, form, seed, n, p, count):
    rc, x = rng_eval(gpu, form, seed, count, cnt=np.full(count, n, np.uint32), a=np.full(count, p))
    assert rc == 0
    return x


def draw_host(H, form, seed, n, p, count):
    x = np.zeros(count, np.uint32)
    (H.draw_binomial if form == BINOMIAL else H.draw_binomial_by_inversion)(seed, n, p, count, x.ctypes.data)
    return x


N = 60000                                                                # _check_against_scipy's


@pytest.fixture(scope="module")
def device_draws(gpu):
    """(form, n, p) -> 60000 device draws with the harness's seeds and streams: seed 12345 + n, stream i; drawn once"""
    out = {}
    for form, cases in ((BINOMIAL, BINOMIAL_CASES), (BINOMIAL_INV, INVERSION_CASES)):
        for n, p in cases:
            out[(form, n, p)] = draw_device(gpu, form, 12345 + n, n, p, N)
    return out


# ---- words and uniforms ----
def test_philox_words_are_the_hosts(gpu, H):
    """the three Random123 known answers of test_philox_known_answers from the device's block(); then the first 4099 words of next32()
    (not a multiple of 4: the last block is read in part) for streams and substreams below, at and above 2^32, bit for bit"""
    kat = [((0, 0), (0, 0, 0, 0), ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]),
           ((0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF,) * 4, ["0x408f276d", "0x41c83b0e", "0xa20bc7c6", "0x6d5451fd"]),
           ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), ["0xd16cfe09", "0x94fdcceb", "0x5001e420", "0x24126ea1"])]
    for key, ctr, want in kat:
        rc, out = rng_eval(gpu, BLOCK, key[0] | key[1] << 32, 1, stream=[ctr[0] | ctr[1] << 32], sub=[ctr[2] | ctr[3] << 32])
        assert rc == 0 and [hex(x) for x in out] == want
    ids = [0, 1, 5, (1 << 32) - 1, 1 << 32, (1 << 32) + 5, (1 << 40) + 3, (1 << 64) - 1]
    stream = np.array([s for s in ids for _ in ids], np.uint64); sub = np.array([b for _ in ids for b in ids], np.uint64)
    w = 4099
    for seed in (77, (0xC0FFEE << 32) | 9):
        rc, got = rng_eval(gpu, WORDS, seed, len(stream), stream=stream, sub=sub, w=w)
        assert rc == 0
        want = np.zeros((len(stream), w), np.uint32)
        for i in range(len(stream)):
            H.draw_words(seed, int(stream[i]), int(sub[i]), w, want[i].ctypes.data)
        assert np.array_equal(got.reshape(len(stream), w), want)
    # without the arrays: stream = the element's index, substream 0
    rc, got = rng_eval(gpu, WORDS, 77, 3, w=7)
    want = np.zeros((3, 7), np.uint32)
    for i in range(3):
        H.draw_words(77, i, 0, 7, want[i].ctypes.data)
    assert rc == 0 and np.array_equal(got.reshape(3, 7), want)


def test_uniforms_are_the_hosts(gpu, H):
    """uniform() bit for bit: 4097 draws (two words each; 4097 is odd, so the last block is half read) of the (stream, substream)
    pairs of test_sequences_share_no_block"""
    pairs = [(st, sb) for st in (5, 6, (1 << 32) | 5) for sb in (0, 1, 2, 3, 1 << 32, (1 << 32) + 1)]
    w = 4097
    rc, got = rng_eval(gpu, UNIFORM, 77, len(pairs), stream=[p[0] for p in pairs], sub=[p[1] for p in pairs], w=w)
    assert rc == 0
    want = np.zeros((len(pairs), w))
    for i, (st, sb) in enumerate(pairs):
        H.draw_uniform_sub(77, st, sb, w, want[i].ctypes.data)
    assert np.array_equal(got.reshape(len(pairs), w), want) and got.min() > 0.0 and got.max() < 1.0


# ---- ratio_of ----
def _spacings(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_ratio_of_against_the_division(gpu):
    """ratio_of(1, b) within 1 spacing of numpy's 1 / b (what test_gpu_vbmath.test_fast_rcp measured for the same construction), ratio_of(a, b)
    within 2 of a / b: a reciprocal within 2^-52 relative times one rounded product (2^-53) is <= 1.5 * 2^-52 relative, at most 2 ulp.
    Grid: r / (1 - r) for r log-uniform in [1e-12, 0.5] (what binv forms), and a <= b log-uniform in [2^-500, 2^500] (Gibbs reaches
    about [1e-21, 1e11]).
    Measured on an MI355X (printed below): ratio_of(1, b) equals 1 / b on all 65 536 points (0 spacings); r / (1 - r) and a / b are at
    most 1 spacing off, exact in 64 % and 74 % of the points.
    Mutant (device only, scratch build of the library, run once): the second Newton step removed -- this test fails with 11 spacings
    for 1 / b (at b = 1.39e78), 20 for r / (1 - r) and 18 for a / b.  (The draw-for-draw tests below did not see that mutant: 0 of
    2 580 000 binomial draws and 0 of 2 100 000 chain draws moved -- presumably because a ratio 20 ulp off moves a draw only when a uniform
    falls within ~1e-14 of a CDF boundary.  This test is the one that holds the arithmetic.)"""
    rng = np.random.default_rng(11)
    n = 1 << 16
    r = np.exp(rng.uniform(np.log(1e-12), np.log(0.5), n))
    e1, e2 = rng.uniform(-500, 500, n), rng.uniform(-500, 500, n)
    x, y = np.exp2(e1) * rng.uniform(1, 2, n), np.exp2(e2) * rng.uniform(1, 2, n)
    a, b = np.minimum(x, y), np.maximum(x, y)
    rc, one = rng_eval(gpu, RATIO, 0, n, a=np.ones(n), b=b)
    assert rc == 0
    k1 = _spacings(one, 1.0 / b)
    rc, odds = rng_eval(gpu, RATIO, 0, n, a=r, b=1.0 - r)
    assert rc == 0
    rc, gen = rng_eval(gpu, RATIO, 0, n, a=a, b=b)
    assert rc == 0
    k2, k3 = _spacings(odds, r / (1.0 - r)), _spacings(gen, a / b)
    print(f"ratio_of: max spacings  1/b {k1.max():.3f}   r/(1-r) {k2.max():.3f}   a/b {k3.max():.3f};  exact in {np.mean(k1 == 0):.4f} / {np.mean(k2 == 0):.4f} / {np.mean(k3 == 0):.4f}")
    assert k1.max() <= 1.0, (k1.max(), b[np.argmax(k1)])
    assert k2.max() <= 2.0, (k2.max(), r[np.argmax(k2)])
    assert k3.max() <= 2.0, (k3.max(), a[np.argmax(k3)], b[np.argmax(k3)])


def test_ratio_of_domain(gpu):
    """The contract of ratio_of (rng.h; sfgpu_gibbs_sample's comment in sfgpu.h): b normal and finite with a normal reciprocal,
    2^-1022 <= b <= 2^1022.  Asserted on the border and for a = 0 inside: within 2 spacings, and 0 exactly.
    The rows outside -- a denormal b, b > 2^1022, b = inf, a = 0 over each, and the chain with all weights scaled by 2^-1060 -- are
    printed and not asserted: the guard that would make them a / b was built and costs the Gibbs kernels registers and spills
    (profiles/gibbs_chain_resource_usage.md), so outside the domain the value is whatever the reciprocal instruction leaves.
    Measured on an MI355X: NaN for b = 1e-310 and b = inf whatever a; the quotient for b = 2^1023; the chain gives [0, 600, 0] in every draw."""
    lo, hi = 2.0 ** -1022, 2.0 ** 1022
    a = np.array([0.3 * lo, lo, 1.0, 0.0, 1.0, 0.25 * hi, hi, 0.0, 0.0])
    b = np.array([lo, lo, lo * 2 ** 60, lo, hi, hi, hi, hi, 3.0])
    rc, got = rng_eval(gpu, RATIO, 0, len(a), a=a, b=b)
    assert rc == 0
    want = a / b
    assert np.all(np.isfinite(want)) and np.all(_spacings(got[want > 0], want[want > 0]) <= 2.0), (got, want)
    assert np.all(got[want == 0] == 0.0)
    ea = np.array([1.0, 1e-310, 0.0, 1.0, 0.0, 1.0, 0.0, 2.0 ** 1023])
    eb = np.array([1e-310, 1e-310, 1e-310, 2.0 ** 1023, 2.0 ** 1023, np.inf, np.inf, 2.0 ** 1023])
    rc, out = rng_eval(gpu, RATIO, 0, len(ea), a=ea, b=eb)
    assert rc == 0
    with np.errstate(all="ignore"):
        print("outside the domain (not asserted): a, b, device, a / b:", [(x, y, g, x / y) for x, y, g in zip(ea, eb, out)])
    w = np.array([3.0, 1.0, 2.0]) * 2.0 ** -1060
    print("chain over weights [3, 1, 2] * 2^-1060, n = 600, last = 0 (not asserted):", chain_device(gpu, w, 600, 0, 0, 5, 4).tolist())


# ---- binomials ----
@pytest.mark.parametrize("n,p", BINOMIAL_CASES)
def test_device_binomial_matches_scipy(device_draws, n, p):
    x = device_draws[(BINOMIAL, n, p)]
    _check_against_scipy(lambda seed, n_, p_, cnt, ptr: C.memmove(ptr, x.ctypes.data, cnt * 4), n, p)


@pytest.mark.parametrize("n,p", INVERSION_CASES)
def test_device_binomial_by_inversion_matches_scipy(device_draws, n, p):
    x = device_draws[(BINOMIAL_INV, n, p)]
    _check_against_scipy(lambda seed, n_, p_, cnt, ptr: C.memmove(ptr, x.ctypes.data, cnt * 4), n, p)


def test_device_binomial_edges(gpu):
    for form in (BINOMIAL, BINOMIAL_INV):
        for (n, p), want in zip(EDGE_CASES, (0, 0, 77)):
            assert np.all(draw_device(gpu, form, 1, n, p, 10) == want)


def test_device_binomials_are_the_hosts_draw_for_draw(device_draws, H):
    """the 43 x 60000 draws above against the host's for the same (seed, stream, n, p): the pooled share that differs is at most 1e-4,
    and where the mean n min(p, 1 - p) is below 110 -- inversion alone -- a differing draw differs by exactly 1 (a uniform on a CDF
    boundary).  Measured on an MI355X: 0 of 2 580 000 draws differ (printed below)."""
    differ = total = 0
    for (form, n, p), x in device_draws.items():
        h = draw_host(H, form, 12345 + n, n, p, N)
        d = x.astype(np.int64) - h.astype(np.int64)
        differ += int((d != 0).sum()); total += N
        if n * min(p, 1 - p) < BINV_MAX_MEAN:
            assert np.all(np.abs(d[d != 0]) == 1), (form, n, p, d[d != 0][:10])
    print(f"binomial draws that differ from the host's: {differ} of {total} ({differ / total:.2e})")
    assert differ / total <= 1e-4


def test_lanes_do_not_see_each_other(gpu):
    """one launch whose wavefronts each hold EVERY (n, p) of the lists above -- short and long BINV walks, BTPE, the flip p > 0.5, n = 0,
    p = 0, p = 1 side by side -- against launches in which all lanes hold one pair: element for element the same draw"""
    for form, cases in ((BINOMIAL, BINOMIAL_CASES + EDGE_CASES), (BINOMIAL_INV, INVERSION_CASES + EDGE_CASES)):
        k = len(cases); count = 64 * 9 + 17
        assert k <= 32                                            # a wavefront of 64 consecutive elements holds every pair twice
        which = (np.arange(count) + 5 * (np.arange(count) // 64)) % k
        cnt = np.array([cases[j][0] for j in which], np.uint32); p = np.array([cases[j][1] for j in which])
        rc, mixed = rng_eval(gpu, form, 4242, count, cnt=cnt, a=p)
        assert rc == 0
        for j, (n, pj) in enumerate(cases):
            alone = draw_device(gpu, form, 4242, n, pj, count)
            assert np.array_equal(mixed[which == j], alone[which == j]), (form, n, pj)


@pytest.mark.parametrize("form", [WORDS, UNIFORM, RATIO, BINOMIAL, BINOMIAL_INV, BLOCK])
def test_launch_edges(gpu, form):
    """n = 0, 1, below / at / above a wavefront and a block: element i is the same value whatever n, and what lies behind n stays untouched"""
    full_n = 257
    rng = np.random.default_rng(3)
    kw = dict(w=3) if form in (WORDS, UNIFORM) else {}
    if form == RATIO: kw = dict(a=rng.random(full_n), b=rng.random(full_n) + 0.5)
    if form in (BINOMIAL, BINOMIAL_INV): kw = dict(cnt=rng.integers(0, 3000, full_n).astype(np.uint32), a=rng.random(full_n))
    if form == BLOCK: kw = dict(stream=rng.integers(0, 1 << 62, full_n).astype(np.uint64), sub=rng.integers(0, 1 << 62, full_n).astype(np.uint64))
    per = 3 if form in (WORDS, UNIFORM) else (4 if form == BLOCK else 1)
    untouched = (lambda v: np.isnan(v).all()) if form in (UNIFORM, RATIO) else (lambda v: np.all(v == SENTINEL))
    rc, full = rng_eval(gpu, form, 9, full_n, **kw)
    assert rc == 0 and not untouched(full[:per])
    for n in (0, 1, 63, 64, 65, 256, 257):
        cut = {k: (v if k == "w" else v[:max(n, 1)]) for k, v in kw.items()}
        rc, got = rng_eval(gpu, form, 9, n, guard=2, **cut)
        assert rc == 0 and np.array_equal(got[:n * per], full[:n * per]) and untouched(got[n * per:]), (form, n)


def test_unknown_form_is_refused(gpu):
    from sailfish_amd import _lib
    x = np.ones(64)
    for form in (-1, 6, 1 << 20):
        rc, got = rng_eval(gpu, form, 1, 64, cnt=np.ones(64, np.uint32), a=x, b=x, stream=np.arange(64), sub=np.arange(64), w=1, guard=1)
        assert rc == _lib.ERR_INVALID and np.all(got == SENTINEL)
        assert b"sfgpu_rng_eval" in _lib.lib().sfgpu_last_error()
    for light in (-1, 2):
        assert chain_device(gpu, np.array([1.0, 2.0]), 10, 0, light, 1, 8, want_rc=_lib.ERR_INVALID) is None
        assert b"sfgpu_chain_eval" in _lib.lib().sfgpu_last_error()


# ---- the chain ----
def chain_device(gpu, w, n, last, light, seed, count, want_rc=0):
    """-> [count, k] draws, or None when the call is refused (and then nothing was written)"""
    import torch
    from sailfish_amd import _lib
    tw = torch.from_numpy(np.ascontiguousarray(w, np.float64)).to(gpu)
    out = torch.full((count * len(w) + 1,), SENTINEL - (1 << 32), dtype=torch.int32, device=gpu)
    rc = _lib.lib().sfgpu_chain_eval(light, _lib.ptr(tw), len(w), n, last, seed, count, _lib.ptr(out), _lib.current_stream_ptr())
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint32)
    assert rc == want_rc and o[-1] == SENTINEL
    if rc:
        assert np.all(o == SENTINEL)
        return None
    return o[:-1].reshape(count, len(w))


def test_chain_is_the_hosts_draw_for_draw(gpu, H):
    """sfgpu_chain_eval against the harness's draw_chain over test_chain_cpu's cases (both forms, `last` at every position, seed
    777 + last, 60000 draws each): every draw sums to n, and the pooled share of draws -- vectors of k -- that differ is at most 1e-4.
    count = 0 and a launch that ends inside a wavefront leave what lies behind untouched (chain_device's guard word).
    Measured on an MI355X: 0 of 2 100 000 draws differ (printed below)."""
    differ = total = 0
    for _, n, w, last, light in T.chain_runs():
        got = chain_device(gpu, w, n, last, light, 777 + last, T.N_DRAWS)
        assert np.all(got.sum(1, dtype=np.int64) == n)
        differ += int((got != T.host_chain(H, n, w, last, light)).any(1).sum()); total += T.N_DRAWS
    print(f"chain draws that differ from the host's: {differ} of {total} ({differ / total:.2e})")
    assert differ / total <= 1e-4
    assert chain_device(gpu, np.array([1.0, 2.0]), 10, 1, 0, 3, 0).shape == (0, 2)
    assert np.array_equal(chain_device(gpu, np.array([1.0, 2.0]), 10, 1, 1, 3, 65), chain_device(gpu, np.array([1.0, 2.0]), 10, 1, 1, 3, 129)[:65])


# ---- the tree ----
def tree_counts(C_):
    """class counts with a run of empty classes inside the tree and one class of more than 3 000 000 reads (BTPE high in the tree)"""
    rng = np.random.default_rng(C_)
    cnt = rng.integers(0, 200, C_).astype(np.int64)
    if C_ > 3:
        cnt[C_ // 3: C_ // 3 + max(2, C_ // 7)] = 0
    cnt[(2 * C_) // 3] += 3_000_000
    return cnt


@pytest.mark.parametrize("levels", [False, True])
def test_tree_is_the_hosts_vector_for_vector(gpu, H, monkeypatch, levels):
    """sfgpu_mn_tree_eval against the harness's tree_multinomial: C = 1, 2, 3, 2048, 2049 (the first width with a top block that
    splits), 5000; three (seed, draw) pairs; the two-launch form and SFGPU_MN_TREE=levels.  Every vector sums to n_total; at most one
    of the 18 vectors may differ.  Measured on an MI355X: 0 of 18 in either form (printed below)."""
    import torch
    from sailfish_amd import _lib
    if levels: monkeypatch.setenv("SFGPU_MN_TREE", "levels")
    else: monkeypatch.delenv("SFGPU_MN_TREE", raising=False)
    differ = 0
    for C_ in (1, 2, 3, 2048, 2049, 5000):
        cnt = tree_counts(C_)
        prefix = np.zeros(C_ + 1, np.uint64); prefix[1:] = np.cumsum(cnt)
        n_total = int(prefix[-1])
        dp = _u64(gpu, prefix)
        for seed, draw in ((1, 0), (99, 7), ((5 << 40) | 3, (1 << 32) + 2)):
            out = torch.full((C_ + 1,), SENTINEL - (1 << 32), dtype=torch.int32, device=gpu)
            rc = _lib.lib().sfgpu_mn_tree_eval(_lib.ptr(dp), C_, n_total, seed, draw, _lib.ptr(out), _lib.current_stream_ptr())
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint32)
            assert rc == 0 and got[C_] == SENTINEL
            got = got[:C_]
            want = np.zeros(C_, np.uint32)
            H.tree_multinomial(seed, draw, C_, prefix.ctypes.data, n_total, want.ctypes.data)
            assert int(got.sum(dtype=np.int64)) == n_total == int(want.sum(dtype=np.int64)) and not got[cnt == 0].any()
            differ += int(not np.array_equal(got, want))
    print(f"tree vectors that differ from the host's ({'levels' if levels else 'two launches'}): {differ} of 18")
    assert differ <= 1


# ---- Gibbs, chain by chain ----
def gibbs_problem(name):
    """-> (eff[M], mass[M], rowptr, ids, counts): small class tables written down directly
    a: 40 transcripts, 50 classes of 2 - 5 members and at most 1500 reads: one tile, light classes only
    b: a with five counts raised to 2000 .. 400 000: heavy and light classes share the tile
    c: 5000 transcripts, ~400 banded classes in 7 tiles whose bands overlap (K >= 2), light and heavy; 3 classes that span more than
       2048 ids (wide), singleton and empty classes, and transcripts that appear in no class"""
    rng = np.random.default_rng(dict(a=1, b=1, c=3)[name])
    if name in "ab":
        M = 40
        labels = [np.sort(rng.choice(M, int(rng.integers(2, 6)), replace=False)) for _ in range(50)]
        counts = rng.integers(1, 1501, 50)
        if name == "b":
            counts[[3, 17, 18, 40, 49]] = [2000, 400_000, 31_000, 2500, 150_000]
    else:
        M = 5000
        labels, counts = [], []
        for c in range(400):
            base = 12 * c
            k = int(rng.integers(1, 6)) if c % 9 else (1 if c % 2 else 0)           # singletons and empty classes among them
            labels.append(np.sort(base + rng.choice(40, k, replace=False)))
            counts.append(0 if k == 0 else (int(rng.integers(1, 1501)) if c % 23 else int(rng.integers(2000, 90_000))))
        for at, lab in ((50, [600, 640, 4900]), (200, [2400, 2410, 4900, 10]), (399, [4790, 4800, 2700])):     # wide: span > 2048
            labels.insert(at, np.sort(np.array(lab))); counts.insert(at, 700 + at)
        counts = np.array(counts)
    rowptr = np.zeros(len(labels) + 1, np.uint32); rowptr[1:] = np.cumsum([len(l) for l in labels])
    ids = np.concatenate(labels).astype(np.uint32)
    eff = rng.uniform(0.5, 3000.0, M)                                              # below 1: the clamp of k_gibbs_weights
    mass = rng.random(M) * (rng.random(M) > 0.2); mass /= mass.sum()               # a fifth of the transcripts start on the prior alone
    return eff, mass, rowptr, ids, counts.astype(np.uint64)


@pytest.mark.parametrize("n_chains", [64, 128, 70])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_gibbs_is_the_restatement_chain_by_chain(gpu, H, name, n_chains):
    """sfgpu_gibbs_sample, 6 rounds, against the harness's serial restatement (gibbs_serial: the same header, g++) with the plan restated
    in test_chain_cpu.gibbs_plan: every sample sums to R; at most one chain of the run differs from the restatement in any sample, all
    others are equal entry for entry; the same seed twice is bit-equal.  70 chains leave a partly filled group of 64.
    Host against host 0 chains differ; a wrong Philox stream, visiting order or member moves every chain (test_chain_cpu.py's mutants).
    Measured on an MI355X: 0 chains differ in each of the nine runs (printed below); with `a.round + 1` -> `a.round` in the device
    library alone every chain of every run differs."""
    import torch
    import sailfish_amd as sf
    from sailfish_amd import _lib
    eff, mass, rowptr, ids, counts = gibbs_problem(name)
    M, R, rounds, seed = len(eff), int(counts.sum()), 6, 31
    kind, K = T.gibbs_plan(rowptr.astype(np.int64), ids, counts)
    assert (kind == 1).sum() == (3 if name == "c" else 0) and ((kind == 2).sum() > 0) == (name != "a")
    want = T.host_gibbs(H, eff, mass, rowptr, ids, counts, R, n_chains, seed, rounds, kind, K)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(gpu)
    args = (dev(eff, np.float64), dev(mass, np.float64), dev(rowptr, np.int32), dev(ids, np.int32), dev(counts, np.int64), R, rounds * n_chains)
    logs = []
    _lib.set_logger(lambda lvl, msg: logs.append(msg))
    try:
        rc, g = sf.gibbs_sample(*args, n_chains=n_chains, seed=seed)
    finally:
        _lib.set_logger(None)
    assert rc == 0
    plan = [m for m in logs if "gibbs:" in m][-1]                 # "gibbs: N chains, H heavy tiles, T tiles in K phases, W wide classes"
    assert int(plan.split(" tiles in ")[1].split()[0]) == K and (K >= 2) == (name == "c"), (plan, K)
    assert int(plan.split(" phases, ")[1].split()[0]) == (kind == 1).sum() and "colours" not in plan and "thin" not in plan, plan
    assert (int(plan.split(" chains, ")[1].split()[0]) > 0) == (name != "a"), plan
    got = g.cpu().numpy()
    assert np.all(got.sum(1, dtype=np.int64) == R) and got.min() >= 0
    never = np.ones(M, bool); never[ids] = False
    assert never.any() == (name == "c") and not got[:, never].any()
    bad = np.unique(np.nonzero((got != want).any(1))[0] % n_chains)
    print(f"gibbs {name}, {n_chains} chains: {len(bad)} chains differ from the restatement")
    assert len(bad) <= 1, bad
    rc, g2 = sf.gibbs_sample(*args, n_chains=n_chains, seed=seed)
    assert rc == 0 and torch.equal(g, g2)
