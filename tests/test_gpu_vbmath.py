"""GPU tests (-m gpu) of the VBEM x arithmetic (sailfish_amd/csrc/vbmath.h) per evaluation: every form of
x_t = exp(psi(alpha_t) - c) / effLen_t through sfgpu_vb_eval, one lane per element, against tests/golden/vbmath_vectors.npz (mpmath at
60 digits, rounded once) under the bounds of tests/test_vbmath_cpu.py -- the same shape, the same K and K0, measured there on the
host forms -- and the loops that call the forms against the same recurrences in mpmath on problems small enough for it.

The mutants of test_vbmath_cpu.py's table reach the device through the same header for forms 0 - 3.  vb_x_head has constants of its
own (literals) and no host twin: `1.0 / 240.0 -> 1.0 / 252.0` applied to ITS series literal in a scratch build and
test_device_forms_against_mpmath run once on the device is the check that this bound sees its constants too (figure in that test)."""

import numpy as np
import pytest

import test_vbmath_cpu as V
from test_vbmath_cpu import K_PSI, K_X

pytestmark = pytest.mark.gpu

DIGAMMA, X_PREPARE, X_LEAN, X_FAST, X_HEAD, RCP = range(6)          # include/sfgpu.h: SFGPU_VB_*
X_FORMS = {X_PREPARE: "exp(digamma_pos - c) / len", X_LEAN: "vb_x_lean", X_FAST: "vb_x_fast", X_HEAD: "vb_x_head"}


@pytest.fixture(scope="module")
def Z():
    return V.load_vectors()


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return V.build_harness(tmp_path_factory)


def vb_eval(gpu, form, a=None, c=None, length=None, n=None, guard=0):
    """-> (rc, out[n + guard] as numpy; NaN where the kernel did not write)"""
    import torch
    from sailfish_amd import _lib
    dev = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, np.float64)).to(gpu)
    ta, tc, tl = dev(a), dev(c), dev(length)
    if n is None:
        n = len(a if a is not None else length)
    out = torch.full((n + guard,), float("nan"), dtype=torch.float64, device=gpu)
    rc = _lib.lib().sfgpu_vb_eval(form, _lib.ptr(ta), _lib.ptr(tc), _lib.ptr(tl), n, _lib.ptr(out), _lib.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


@pytest.fixture(scope="module")
def device_x(gpu, Z):
    """every x form over the whole grid, once"""
    out = {}
    for f in X_FORMS:
        rc, g = vb_eval(gpu, f, Z["x_a"], Z["x_c"], Z["x_len"])
        assert rc == 0
        out[f] = g
    return out


@pytest.mark.parametrize("form", list(X_FORMS))
def test_device_forms_against_mpmath(device_x, Z, form):
    """Measured on an MI355X against the host's K = 31: exp(digamma_pos - c) / len 13.76, vb_x_lean 15.48, vb_x_fast 15.48, vb_x_head
    15.48 (digamma_pos: K0 3.12) -- the host's figures to the digit, at the same points.  vb_x_head needs no K of its own: its reciprocal
    is not IEEE, but two Newton steps leave it within an ulp (test_fast_rcp) of a quantity whose own rounding the shape already carries.
    With `1.0 / 240.0 -> 1.0 / 252.0` in vb_x_head's literal (scratch build, run once) this test fails for form 4 alone with
    K = 1.6e4 at a = 10, c = psi(11), len = 1 (relative error 2.0e-12), as the host forms do in test_vbmath_cpu.py's table."""
    k, i = V.x_excess(device_x[form], Z)
    print(f"{X_FORMS[form]}: measured K = {k:.3f} at a = {Z['x_a'][i]!r}, c = {Z['x_c'][i]!r}, len = {Z['x_len'][i]!r}")
    assert k <= K_X, (X_FORMS[form], k, Z["x_a"][i], Z["x_c"][i], Z["x_len"][i], device_x[form][i], Z["x_want"][i])


def test_device_forms_agree_pairwise(device_x, Z):
    """forms 1, 2, 3 and 4 pairwise within twice the bound on every grid point"""
    lim = 2.0 * K_X * V.x_scale(Z) * Z["x_want"]
    forms = list(X_FORMS)
    for i, f1 in enumerate(forms):
        for f2 in forms[i + 1:]:
            d = np.abs(device_x[f1] - device_x[f2])
            j = int(np.argmax(d / lim))
            assert (d <= lim).all(), (X_FORMS[f1], X_FORMS[f2], Z["x_a"][j], Z["x_c"][j], Z["x_len"][j], device_x[f1][j], device_x[f2][j])


def test_device_digamma_against_mpmath_and_the_host(gpu, Z, H):
    rc, got = vb_eval(gpu, DIGAMMA, Z["psi_x"])
    assert rc == 0
    k, i = V.psi_excess(got, Z)
    print(f"digamma_pos: measured K0 = {k:.3f} at x = {Z['psi_x'][i]!r}")
    assert k <= K_PSI, (k, Z["psi_x"][i], got[i], Z["psi_want"][i])
    host = V.host_eval(H, DIGAMMA, Z["psi_x"])
    fin = np.isfinite(Z["psi_want"])
    assert np.array_equal(got[~fin], host[~fin])
    assert (np.abs(got[fin] - host[fin]) <= 2.0 * K_PSI * V.psi_scale(Z)[fin]).all()


def test_fast_rcp(gpu, Z):
    """form 5 within 1 ulp of the correctly rounded 1 / x: over the lengths, and over the products d y len whose reciprocal the head
    forms (d = a (a + 1) ... (a + 9) and y = a + 10 below 10, else d = 1 and y = a: [10, 7e18] on this grid), and over a log-uniform
    sweep of [1e-1, 1e26] that holds both with room to spare"""
    a, ln = Z["x_a"], Z["x_len"]
    d = np.where(a < 10.0, np.prod(np.where(a[:, None] < 10.0, a[:, None] + np.arange(10.0), 1.0), axis=1), 1.0)
    prod = d * np.where(a < 10.0, a + 10.0, a) * ln
    assert prod.min() == 10.0 and 1e18 < prod.max() < 1e26
    for x in (ln, prod, np.exp(np.linspace(np.log(1e-1), np.log(1e26), 4096))):
        rc, got = vb_eval(gpu, RCP, length=x)
        want = 1.0 / x
        assert rc == 0 and (np.abs(got - want) <= np.spacing(want)).all(), float(np.max(np.abs(got - want) / np.spacing(want)))


@pytest.mark.parametrize("form", [DIGAMMA, X_LEAN, X_HEAD, RCP])
def test_launch_edges(gpu, Z, device_x, form):
    """n = 0, 1, below / at / above a wavefront and a block, the full grid: element i is the same value whatever n, and the element
    behind n stays untouched"""
    a, c, ln = Z["x_a"], Z["x_c"], Z["x_len"]
    rc, full = vb_eval(gpu, form, a, c, ln)
    assert rc == 0 and not np.isnan(full).any()
    if form in device_x:
        assert np.array_equal(full, device_x[form])
    for n in (0, 1, 63, 64, 65, 256, 257, len(a)):
        rc, got = vb_eval(gpu, form, a[:max(n, 1)], c[:max(n, 1)], ln[:max(n, 1)], n=n, guard=1)
        assert rc == 0 and np.array_equal(got[:n], full[:n]) and np.isnan(got[n]), (form, n)


def test_unknown_form_is_refused(gpu, Z):
    from sailfish_amd import _lib
    for form in (-1, 6, 1 << 20):
        rc, got = vb_eval(gpu, form, Z["x_a"][:64], Z["x_c"][:64], Z["x_len"][:64], guard=1)
        assert rc == _lib.ERR_INVALID and np.isnan(got).all()
        assert b"sfgpu_vb_eval" in _lib.lib().sfgpu_last_error()


# ---- the loops that call the forms, against mpmath ----
LOOPS = {"two": dict(SFGPU_EM_FUSED="0"), "fused": dict(SFGPU_EM_FUSED="1", SFGPU_EM_PERSIST="0"),
         "persist": dict(SFGPU_EM_FUSED="1", SFGPU_EM_PERSIST="1")}


@pytest.mark.parametrize("vb", [False, True])
@pytest.mark.parametrize("loop", list(LOOPS))
@pytest.mark.parametrize("name", ["toy5", "toy7", "rand", "lowdepth"])
def test_loops_against_mpmath(gpu, Z, monkeypatch, name, loop, vb):
    """the fixture's small problems through EMProblem.optimize(tol = 0, min_iter = max_iter = n) in each loop form (a new handle per
    form: the switches are read when the plan is made), n = 1, 2, 7, against em_numpy_restatement.optimize_mp from the fixture.
    The bar is test_em_independent.test_oracle_and_numpy_agree_with_mpmath_on_small_problems': rtol 1e-11 on the entries above the
    truncation cutoff.  `lowdepth` starts at alpha = 3 / 700 below the prior: its first x comes from the full digamma_pos."""
    import torch
    import sailfish_amd as sf
    for k in ("SFGPU_EM_FUSED", "SFGPU_EM_PERSIST"): monkeypatch.delenv(k, raising=False)
    for k, v in LOOPS[loop].items(): monkeypatch.setenv(k, v)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(gpu)
    eff, rp, ii, cc, N = (Z[f"p_{name}_{k}"] for k in ("eff", "rp", "ii", "cc", "N"))
    g = sf.EMProblem(torch.from_numpy(np.ascontiguousarray(eff, dtype=np.float64)).to(gpu), t(rp.astype(np.uint32), np.int32),
                     t(ii.astype(np.uint32), np.int32), t(cc.astype(np.uint64), np.int64), int(N))
    try:
        for n in (1, 2, 7):
            ref = Z[f"p_{name}_{'vb' if vb else 'em'}_{n}"]
            rc, st = g.optimize(use_vbem=vb, tol=0.0, min_iter=n, max_iter=n)
            assert rc == 0 and st["iters"] == n
            assert (bool(st["fused"]), bool(st["persistent"])) == dict(two=(False, False), fused=(True, False), persist=(True, True))[loop], st
            a = g.alpha.cpu().numpy()
            cutoff = (0.01 + 1e-8) if vb else 1e-8                # optimize() returns the truncated vector
            keep = ref > cutoff * (1 + 1e-6)
            assert keep.any()
            print(f"{name} {loop} {'VBEM' if vb else 'EM'} n = {n}: max rel {float(np.max(np.abs(a[keep] - ref[keep]) / ref[keep])):.3g}")
            np.testing.assert_allclose(a[keep], ref[keep], rtol=1e-11)
    finally:
        g.close()
