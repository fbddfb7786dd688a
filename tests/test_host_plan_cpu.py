"""CPU: the host-side launch planners of bagel_amd/csrc/host_plan.cpp -- plain C++ with no HIP in it, so it is checked twice without a GPU:
a stand-alone fuzz program (tests/host_plan_fuzz.cpp) linked against that one file runs under ASan + UBSan as a child process, and the library
build of the same file must reproduce the schedules recorded before the planners moved there (tests/golden/host_plan_parent.json)."""
import ctypes
import hashlib
import json
import os
import shutil
import subprocess
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build_fuzz(out):
    """Whichever of g++ / the ROCm clang++ links the sanitizer runtimes (statically: the program needs nothing preloaded); else an unsanitized build."""
    srcs = [os.path.join(ROOT, "tests", "host_plan_fuzz.cpp"), os.path.join(ROOT, "bagel_amd", "csrc", "host_plan.cpp")]
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
    warnings.warn("host_plan_fuzz runs UNSANITIZED: no compiler here links ASan + UBSan (" + " | ".join(tried) + ")")
    return False


def test_host_plan_fuzz_under_asan_ubsan(tmp_path):
    """2 005 attention plans (coverage exactly once, slots written / read once, ops.AttnPlan's capacity formula, exact-size and one-short heap buffers),
    the K-split grid of the persistent GEMM, every gemv_mb row length up to 32 768 (incl. the workspace bound) and random decode-engine chains."""
    exe = str(tmp_path / "host_plan_fuzz")
    _build_fuzz(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "ok" in r.stdout


def _starts(lens, align=1):
    out, c = [], 0
    for n in lens:
        out.append(c)
        c += (max(n, 1) + 63) // 64 * 64 if align == 64 else n
    return out


def test_schedules_equal_the_recorded_ones():
    """Same schedule as before the move: sha256 of the plan buffer bagel_attn_plan writes for 40 seeded geometries + the benchmark's five launches, and
    bagel_gemv_mb_workspace_bytes over the models' row lengths, recorded from the library of the commit before host_plan.cpp existed."""
    from bagel_amd import _lib
    L = _lib.lib()
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "host_plan_parent.json")))
    assert len(doc["attn_plans"]) == 45
    for g in doc["attn_plans"]:
        q_len, ctx_len = g["q_len"], g["ctx_len"]
        i32 = lambda x: np.ascontiguousarray(np.asarray(list(x) + [0], dtype=np.int32))  # noqa: E731
        a = [i32(_starts(q_len)), i32(q_len), i32(_starts(ctx_len or [])), i32(ctx_len or []), i32(_starts(q_len, 64)), i32(_starts(ctx_len or [], 64))]
        p = lambda i: a[i].ctypes.data if (ctx_len is not None or i in (0, 1, 4)) else None  # noqa: E731
        buf = np.full(g["used"], -7, dtype=np.int32)
        rc = L.bagel_attn_plan(p(0), p(1), p(2), p(3), p(4), p(5), len(q_len), g["nq"], g["nkv"], int(g["causal"]), g["n_workers"], g["split_min_tiles"],
                               buf.ctypes.data, g["used"])
        assert rc == 0, (g, L.bagel_hip_last_error())
        assert int(buf[5]) + 8 * int(buf[2]) == g["used"] and hashlib.sha256(buf.tobytes()).hexdigest() == g["sha256"], g
    for N, K, want in doc["gemv_mb_workspace_bytes"]:
        out = ctypes.c_int64(-1)
        assert L.bagel_gemv_mb_workspace_bytes(N, K, ctypes.byref(out)) == 0 and out.value == want, (N, K, out.value, want)
