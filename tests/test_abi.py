"""CPU tests of the boundary: the shared library builds for gfx950, loads, and exports exactly the
symbols include/sfgpu.h declares; no compute is possible without a GPU and it says so."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "sfgpu.h")).read()
    return sorted(set(re.findall(r"SFGPU_API [a-z_ *]+?\b(sfgpu_[a-z0-9_]+)\(", txt)))


def test_header_symbols_exported(built):
    so = os.path.join(ROOT, "sailfish_amd", "csrc", "libsfgpu.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    exported = sorted(set(re.findall(r" T (sfgpu_[a-z0-9_]+)", out)))
    decl = _declared()
    assert len(decl) >= 28
    assert exported == decl


def test_python_binding_matches_header(built):
    from sailfish_amd import _lib
    assert _lib.exported_symbols() == _declared()
    L = _lib.lib()
    assert L.sfgpu_version() == 100


def test_header_is_plain_c(built, tmp_path):
    """the boundary is a C ABI: the header must compile as C with no HIP/torch in sight"""
    src = tmp_path / "t.c"
    src.write_text('#include "sfgpu.h"\nint main(void){ sfgpu_problem p; sfgpu_em_opts o; (void)p; (void)o; return SFGPU_OK; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_samw_batch_layout_matches_ctypes(built, tmp_path):
    """sfgpu_samw_batch as gcc lays it out and its ctypes mirror _lib.SamwBatch: the same size, the same offset for every field"""
    from sailfish_amd import _lib
    names = [n for n, _ in _lib.SamwBatch._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sfgpu.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(sfgpu_samw_batch));\n'
                   + "".join(f'    printf("%zu\\n", offsetof(sfgpu_samw_batch, {n}));\n' for n in names) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(_lib.SamwBatch)] + [getattr(_lib.SamwBatch, n).offset for n in names]


def test_sam_write_text_refuses_a_null_batch(built):
    """batch == NULL is SFGPU_ERR_INVALID, before anything touches a device"""
    from sailfish_amd import _lib
    L = _lib.lib()
    res = _lib.SamWriteResult()
    assert L.sfgpu_sam_write_text(None, 0, _lib.TEXT_SINK(0), None, C.byref(res), None) == _lib.ERR_INVALID
    assert b"batch" in L.sfgpu_last_error()


def test_library_links_only_hip_runtime(built):
    so = os.path.join(ROOT, "sailfish_amd", "csrc", "libsfgpu.so")
    out = subprocess.check_output(["readelf", "-d", so], text=True)
    needed = re.findall(r"NEEDED.*\[(.*?)\]", out)
    assert any(n.startswith("libamdhip64") for n in needed)
    assert not any("torch" in n or "c10" in n or "oracle" in n for n in needed)


def test_no_cpu_fallback_without_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from sailfish_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.sfgpu_eq_create(C.byref(h), 0, None)
    assert rc == _lib.ERR_HIP and b"device" in L.sfgpu_last_error().lower()


def test_product_never_imports_oracle():
    """oracle/ is test infrastructure: nothing under sailfish_amd/ may reference it"""
    pkg = os.path.join(ROOT, "sailfish_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".h", ".cpp")) or fn == "Makefile":
                txt = open(os.path.join(dp, fn), errors="replace").read()
                assert "oracle" not in txt.lower(), os.path.join(dp, fn)


def test_cf_tables_host_side(built):
    """the correction tables are host-side serial prefix sums: callable without a GPU, bit-equal to the oracle"""
    import numpy as np
    from oracle import oracle as O
    from sailfish_amd import SailfishOpts, efflen
    np.testing.assert_array_equal(efflen.normal_cf(SailfishOpts()), O.cf_gaussian())
    np.testing.assert_array_equal(efflen.normal_counts(SailfishOpts()), O.fld_gaussian_counts())
    fl = O.fld_gaussian_counts().astype(np.uint32)
    np.testing.assert_array_equal(efflen.counts_cf(fl), O.cf_counts(fl))


def _build_c_host(tmp_path):
    exe = tmp_path / "c_abi_smoke"
    csrc = os.path.join(ROOT, "sailfish_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "c_abi_smoke.c"), "-o", str(exe),
                           "-L", csrc, "-lsfgpu", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + csrc + ",-rpath,/opt/rocm/lib"])
    return exe


def test_c_host_links_against_the_abi(built, tmp_path):
    """a plain-C program (no Python, no torch) compiles and links against libsfgpu"""
    exe = _build_c_host(tmp_path)
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_c_host_runs_the_toy_kat(built, tmp_path):
    """...and reproduces the SURVEY 8c EM known answer when run on the GPU box"""
    exe = _build_c_host(tmp_path)
    out = subprocess.check_output([str(exe)], text=True)
    f = out.split()
    assert f[1] == "50"
    got = [float(x) for x in f[3:7]]
    want = [417.47751898139057, 0.0, 67.522481018609454, 0.0]
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-12 * max(1.0, abs(w))
    assert abs(float(f[8]) - 1e6) < 1e-3
    assert "extras ok" in out        # bootstrap / Gibbs hooks, effective-length helpers and hit filtering, called from C


def _build_cpp_host(tmp_path):
    exe = tmp_path / "cpp_host_test"
    csrc = os.path.join(ROOT, "sailfish_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp_host_test.cpp"), "-o", str(exe),
                           "-L", csrc, "-lsfgpu", "-L", "/opt/rocm/lib", "-lamdhip64", "-pthread",
                           "-Wl,-rpath," + csrc + ",-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_host_adaptor_compiles(built, tmp_path):
    """include/sfgpu_sailfish.hpp -- the reference's classes over the C ABI -- and reference-style host code against
    it compile with g++ (no Boost / TBB / spdlog / Eigen)"""
    assert os.path.exists(_build_cpp_host(tmp_path))


@pytest.mark.gpu
def test_cpp_host_adaptor_runs(built, tmp_path):
    """mapping threads -> addGroup -> finish -> optimize / gatherBootstraps / sample from C++, against the SURVEY 8c
    known answers of the reference's own optimize() and a std::map"""
    exe = _build_cpp_host(tmp_path)
    r = subprocess.run([str(exe)], text=True, capture_output=True)
    assert r.returncode == 0 and "cpp host ok" in r.stdout, r.stdout + r.stderr
