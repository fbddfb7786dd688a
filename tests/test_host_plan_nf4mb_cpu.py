"""CPU: the launch planner of the NF4 batched-decode stream (mbnf4_plan / mbnf4_wave_groups in bagel_amd/csrc/host_plan.cpp + host_plan.h) -- plain C++ with no
HIP in it, checked twice without a GPU as tests/test_host_plan_w4mb_cpu.py checks its sibling: a stand-alone fuzz program (tests/host_plan_nf4mb_fuzz.cpp) linked
against that one file runs under ASan + UBSan as a child process, and the library's entry points are held to the same invariants at the 7B shapes."""
import ctypes
import os
import shutil
import subprocess
import warnings

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build_fuzz(out):
    """Whichever of g++ / the ROCm clang++ links the sanitizer runtimes (statically: the program needs nothing preloaded); else an unsanitized build."""
    srcs = [os.path.join(ROOT, "tests", "host_plan_nf4mb_fuzz.cpp"), os.path.join(ROOT, "bagel_amd", "csrc", "host_plan.cpp")]
    tried = []
    for cxx, extra in (("g++", ["-static-libasan", "-static-libubsan"]), ("/opt/rocm/llvm/bin/clang++", ["-static-libsan"]), ("clang++", ["-static-libsan"])):
        cxx = shutil.which(cxx)
        if cxx:
            r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra"] + SAN + extra + srcs + ["-o", out], capture_output=True, text=True)
            if r.returncode == 0:
                return True
            tried.append(f"{cxx}: {r.stderr[-300:]}")
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + srcs + ["-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    warnings.warn("host_plan_nf4mb_fuzz runs UNSANITIZED: no compiler here links ASan + UBSan (" + " | ".join(tried) + ")")
    return False


def test_nf4mb_plan_fuzz_under_asan_ubsan(tmp_path):
    """Every K multiple of 128 up to 32 768 x N in {16, 32, 48, 64, 4608, 37888} x M in {1, 5, 16, 17, 32} x both epilogues x five workgroup counts: every k-group
    covered exactly once across waves and slices, no empty slice, GP in {1, 2, 4}, gx within the unit count, the slab bound of workspace_bytes, refusals that
    leave no partial plan."""
    exe = str(tmp_path / "host_plan_nf4mb_fuzz")
    _build_fuzz(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.startswith("ok")


def _wave_groups(per, slice_groups, G, s, w):
    """mbnf4_wave_groups (host_plan.h) restated from the entry point's outputs: per / slice_groups k-groups of 128 weights per wave / slice."""
    lo = s * slice_groups + w * per
    hi = min(lo + per, (s + 1) * slice_groups, G)
    return (lo, hi - lo) if lo < hi else (lo, 0)


@pytest.mark.parametrize("M", [5, 16, 17, 32])
@pytest.mark.parametrize("N,K,epi", [(4608, 3584, 0), (3584, 3584, 0), (37888, 3584, 3), (3584, 18944, 0)])
def test_library_geometry_at_7b_shapes(M, N, K, epi):
    from bagel_amd import _lib
    L = _lib.lib()
    ws = ctypes.c_int64(-1)
    assert L.bagel_gemv_mb_nf4_workspace_bytes(N, K, ctypes.byref(ws)) == 0
    G = K // 128
    for wgs in (8, 256, 304):
        per, sg, ks, gx = (ctypes.c_int32(-1) for _ in range(4))
        assert L.bagel_gemv_mb_nf4_geometry(M, N, K, epi, wgs, ctypes.byref(per), ctypes.byref(sg), ctypes.byref(ks), ctypes.byref(gx)) == 0, L.bagel_hip_last_error()
        per, sg, ks, gx = per.value, sg.value, ks.value, gx.value
        assert 1 <= per <= 4 and 1 <= sg <= 8 * per and ks >= 1 and 1 <= gx <= N // (32 if epi == 3 else 16)
        assert (ks == 1) == (K <= 4096)
        cover = [0] * G
        empty = 0
        for s in range(ks):
            in_slice = 0
            for w in range(8):
                g0, ng = _wave_groups(per, sg, G, s, w)
                assert 0 <= ng <= per
                in_slice += ng
                for k in range(g0, g0 + ng):
                    cover[k] += 1
            empty += in_slice == 0
        assert cover == [1] * G and not empty, (M, N, K, wgs, per, sg, ks)
        assert ks == 1 or ws.value >= ks * (32 if M > 16 else 16) * N * 4, (ks, ws.value)
    assert (ws.value == 0) == (K <= 4096)


def test_library_refusals_without_a_gpu():
    from bagel_amd import _lib, ops
    L = _lib.lib()
    o = (ctypes.c_int32 * 4)(-7, -7, -7, -7)
    a = ctypes.addressof(o)
    for M, N, K, epi, word in ((0, 64, 256, 0, b"M=0"), (33, 64, 256, 0, b"M=33"), (8, 64, 192, 0, b"K=192"), (8, 40, 256, 0, b"N=40"), (8, 48, 256, 3, b"N=48"),
                               (8, 64, 256, 1, b"epilogue 1")):
        assert L.bagel_gemv_mb_nf4_geometry(M, N, K, epi, 256, a, a + 4, a + 8, a + 12) == -1 and word in L.bagel_hip_last_error(), (M, N, K, epi)
        assert list(o) == [-7] * 4
    assert ops.MB_NF4_MAX_ROWS == 32
    assert ops.mb_nf4_workspace_floats(3584, 3584) == 0 and ops.mb_nf4_workspace_floats(3584, 18944) * 4 >= 10 * 32 * 3584 * 4
