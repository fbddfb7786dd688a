"""Every matrix-product path on the designed inputs of tests/util_gemm_ref.py: exact families bit for bit, real-valued families inside
the per-element float64 bound (+ the two-rounding membership with a residual), outputs pre-filled with NaN / sentinels.

Paths: ops.gemm variants 0-5 (tile kernels, ping-pong, persistent + K-split at the default grid), the persistent kernel and its K-split
on small grids in child processes (the grid is read once per process), gemm_skinny, the lane-FMA gemv (with and without the fused
RMSNorm), gemv_mb (one / two request blocks, K slices, fused norm), the routing of ops.gemm(variant=None), and the fp8 persistent
kernel.  gemm_w4 and the int8 / nf4 / w4 gemvs are not covered here.

The fused RMSNorm of gemv and gemv_mb runs on the ``exact`` family only, by design: only rows of +-1 keep the norm itself exact (rms 1,
rsqrt(1 + 1e-6) rounds to 1 in bf16, weight +-1), so the fused result must equal the unfused one bit for bit; on any other family the
norm's own rounding would need a bound of its own and this module's reference has none.  gemv_mb runs it where its geometry allows a
norm (one K slice).

Every test prints its worst err / bound (real-valued families; the exact families are bit-equal or fail)."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import util_gemm_ref as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda"
REAL = ("scaled", "cancel", "edges")
ALL = R.EXACT_FAMILIES + REAL


def ops():
    from bagel_amd import ops as o
    return o


@functools.lru_cache(maxsize=8)
def built(family, M, N, K, epi):
    case = R.build(family, M, N, K, epi)
    return case, R.reference(case)


def n_for(N, epi, mult=32):
    return -(-N // mult) * mult if epi == "swiglu" else N


# ------------------------------------------------------------------------------------------------------------
# ops.gemm variants 0-5
# ------------------------------------------------------------------------------------------------------------
# M on both sides of the 128- and 256-row tiles; N: ragged 128 / 256 tiles and the 16-byte store fallback (N = 8, 136, 264, 520 are no
# multiples of 16 -> SwiGLU rounds N up to 32); K = 8 / 72: tail only / one tile + tail (3-5 fall back to the plain 256 x 256 kernel),
# 64: below the persistent kernel's K >= 128, 128 / 192 / 704 / 1152: even and odd k-tile counts of the two-stage ring
GEMM_SHAPES = [(1, 8, 8), (127, 136, 72), (129, 264, 64), (257, 520, 128), (1100, 264, 192), (257, 136, 704), (1100, 520, 1152)]


@pytest.mark.parametrize("epi", R.EPILOGUES)
@pytest.mark.parametrize("family", ALL)
def test_gemm_variants(family, epi):
    o = ops()
    worst = {}
    for M, N, K in GEMM_SHAPES:
        N = n_for(N, epi)
        case, ref = built(family, M, N, K, epi)
        args = R.gemm_args(case, DEV)
        first = None
        for variant in (0, 1, 2, 3, 4, 5):
            reps = 4 if variant >= 3 else 1                      # hand-counted DMA waits: any differing bit between repeats is a race
            outs = [R.run_gemm(o, case, args, variant) for _ in range(reps)]
            if variant >= 4:
                outs.append(R.run_gemm(o, case, args, variant, splitk=False))
            what = f"variant {variant}"
            q = R.assert_case(case, outs[0], ref, what=what)
            worst[variant] = max(worst.get(variant, 0.0), q)
            for x in outs[1:reps]:
                assert torch.equal(R.bits(outs[0]), R.bits(x)), f"{case.name} {what}: repeats differ"
            if variant >= 4:
                if case.exact:
                    assert torch.equal(R.bits(outs[0]), R.bits(outs[-1])), f"{case.name} {what}: split and unsplit schedules differ on exact inputs"
                else:
                    worst[variant] = max(worst[variant], R.assert_case(case, outs[-1], ref, what=what + " unsplit"))
            if case.exact:                                       # also where an activation leaves no single legal pattern: one silu_f / gelu_tanh_f on one input
                first = outs[0] if first is None else first
                assert torch.equal(R.bits(first), R.bits(outs[0])), f"{case.name}: {what} differs from variant 0 on exact inputs"
    print(f"gemm {family}/{epi}: " + ("exact" if family in R.EXACT_FAMILIES and epi not in ("bias_gelu", "silu", "swiglu") else
                                      "worst err / bound " + " ".join(f"v{v} {q:.3f}" for v, q in worst.items())))


# ------------------------------------------------------------------------------------------------------------
# persistent kernel + K-split on small grids (child processes)
# ------------------------------------------------------------------------------------------------------------
GRIDS = {"wgs8_split": dict(BAGEL_GEMM_PERSIST_WGS="8", BAGEL_GEMM_SPLITK="1"), "wgs8_nosplit": dict(BAGEL_GEMM_PERSIST_WGS="8", BAGEL_GEMM_SPLITK="0"),
         "default": dict()}
# (M, N, K) -> (tiles, tiles in full rounds, K parts) of the dense launches on 8 workgroups: 10 tiles / 2 left over / 11 k-tiles -> 2 parts;
# 18 k-tiles -> 4 parts; 15 tiles / 7 left over -> not split; 4 tiles, a single partial round of 16 k-tiles -> 2 parts.  tests/test_gemm_ref_cpu.py
# holds these to the host rule (bagel_gemm_leftover_split); the child processes below report what each launch wrote into the K-split workspace
CLAIMED_WGS8 = {(1100, 264, 704): [10, 8, 2], (1100, 264, 1152): [10, 8, 4], (1100, 520, 1152): [15, 15, 1], (257, 264, 1024): [4, 0, 2]}


def run_grid(grid, family):
    """One fresh child process on ``grid`` -> {(family, epilogue, shape): record}; the child has checked every case and repeat already."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("BAGEL_GEMM_PERSIST_WGS", "BAGEL_GEMM_SPLITK", "BAGEL_GEMM_SPLIT_POLICY", "BAGEL_GEMM_SPLIT_FORCE")}
    env.update(GRIDS[grid])
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "gemm_designed_check.py"), family], env=env, capture_output=True, text=True, timeout=240)
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    bad = [x for x in recs if not x["ok"]]
    assert r.returncode == 0 and "ALL DESIGNED OK" in r.stdout and not bad, grid + ": " + json.dumps(bad, indent=1)[:4000] + r.stdout[-1500:] + r.stderr[-2000:]
    assert len(recs) == 4 * 8 * len(family.split(","))
    print(f"persistent {grid} {family}: " + ("exact" if family in R.EXACT_FAMILIES else f"worst err / bound {max(x['worst'] for x in recs):.3f}"))
    return {(x["family"], x["epi"], tuple(x["shape"])): x for x in recs}


@pytest.mark.parametrize("family", ["exact", "kprobe", "roundpoint", "scaled,cancel", "edges"])
def test_gemm_persistent_grids(family):
    """The three grids one after the other, each in a child of its own, then the comparisons across them."""
    split, nosplit, default = [run_grid(grid, family) for grid in ("wgs8_split", "wgs8_nosplit", "default")]
    assert set(split) == set(nosplit) == set(default)
    for key, x in split.items():
        shape, y = key[2], nosplit[key]
        if x["epi"] == "plain":                                      # the K parts each launch left in the workspace are those of the schedule this module claims
            nblk, n_full, s = CLAIMED_WGS8[shape]
            want = (nblk - n_full) * s if s > 1 else 0
            assert x["parts"] == {"4": want, "5": want}, (key, x["parts"], CLAIMED_WGS8[shape])
            assert y["parts"] == {"4": 0, "5": 0}, (key, y["parts"])
        if x["family"] in R.EXACT_FAMILIES:                           # split, unsplit and default-grid results of one exact case: one bit pattern
            assert x["sha"] == y["sha"] == default[key]["sha"], f"{key}: the grids give different bits on exact inputs"
        elif x["epi"] == "plain" and x["family"] == "scaled":
            # ... and seen in the results: on real values the K parts re-associate the leftover tiles' sums, so the 8-workgroup results with and
            # without the split differ in some bit exactly where the launch wrote K parts
            assert (x["sha"] != y["sha"]) == (x["parts"]["5"] > 0), f"{key}: split / unsplit results {'agree' if x['sha'] == y['sha'] else 'differ'}, K parts {x['parts']}"


# ------------------------------------------------------------------------------------------------------------
# skinny.hip, the lane-FMA gemv, gemv_mb.hip
# ------------------------------------------------------------------------------------------------------------
DENSE_EPIS = ("plain", "bias", "res", "bias_res", "bias_gelu", "silu", "swiglu")


def check_dense(fn, family, M, N, K, epi, what, worst, first=None, **extra):
    case, ref = built(family, M, n_for(N, epi), K, epi)
    out = R.run_dense(fn, case, DEV, **extra)
    q = R.assert_case(case, out, ref, what=what)
    worst[0] = max(worst[0], q)
    return case, out


@pytest.mark.parametrize("epi", DENSE_EPIS)
@pytest.mark.parametrize("family", ALL)
def test_gemm_skinny(family, epi):
    o, worst = ops(), [0.0]
    for M in (2, 16, 17, 64):
        for N, K in [(16, 32), (48, 96), (160, 704)]:
            case, out = check_dense(o.gemm_skinny, family, M, N, K, epi, "skinny", worst)
            if case.exact:                                       # the same bits as the 128 x 128 tile kernel
                assert torch.equal(R.bits(out), R.bits(R.run_gemm(o, case, R.gemm_args(case, DEV), 0))), f"{case.name}: skinny differs from variant 0"
    print(f"skinny {family}/{epi}: worst err / bound {worst[0]:.3f}")


def normed(case, seed=0):
    """(A, norm weight) whose fused RMSNorm gives exactly the case's A: rows of +-1 have rms 1, rsqrt(1 + 1e-6) rounds to 1 in bf16
    (decode.hip / gemv_mb.hip `bfround(lo2f(v[e]) * inv) * lo2f(gw[i][e])`), the weight is +-1."""
    g = torch.Generator().manual_seed(100 + seed)
    w = (torch.randint(0, 2, (case.K,), generator=g) * 2 - 1).to(BF16)
    A = case.A * w[None, :]
    assert bool((A.float().abs() == 1).all())
    return A, w.to(DEV)


@pytest.mark.parametrize("epi", DENSE_EPIS)
@pytest.mark.parametrize("family", ALL)
def test_gemv(family, epi):
    o, worst = ops(), [0.0]
    shapes = [(6, 40), (34, 136), (160, 704)] + ([(32, 8192)] if family in ("exact", "scaled") else [])      # K >= 8192: the four-wave split-K form
    for M in (1, 8):
        for N, K in shapes:
            case, out = check_dense(o.gemv, family, M, N, K, epi, "gemv", worst)
            if family == "exact":
                A, w = normed(case)
                out2 = R.run_dense(o.gemv, case, DEV, A=A, norm_w=w, eps=1e-6)
                R.assert_case(case, out2, built(family, M, n_for(N, epi), K, epi)[1], what="gemv + fused RMSNorm")
                assert torch.equal(R.bits(out), R.bits(out2)), f"{case.name}: the fused norm changes bits on exact inputs"
    print(f"gemv {family}/{epi}: worst err / bound {worst[0]:.3f}")


MB_SHAPES = [(64, 128), (48, 448), (528, 1056), (16, 3584)]


@pytest.mark.parametrize("epi", DENSE_EPIS)
@pytest.mark.parametrize("family", ALL)
def test_gemv_mb(family, epi):
    o, worst = ops(), [0.0]
    for M in (1, 16, 17, 32):
        for N, K in MB_SHAPES + ([(160, 4864)] if M == 17 else []):      # (17, 160, 4864): two K slices
            if epi == "swiglu" and (n_for(N, epi) != N or (M > 16 and K > 3584)):
                continue                                         # N = 48, 528, 16: no multiple of 32 (SwiGLU pairs whole 32-column blocks); K slices carry no SwiGLU
            case, out = check_dense(o.gemv_mb, family, M, N, K, epi, "gemv_mb", worst)
            one_slice = M <= 16 or K <= 3584
            if family == "exact" and one_slice:
                A, w = normed(case)
                out2 = R.run_dense(o.gemv_mb, case, DEV, A=A, norm_w=w, eps=1e-6)
                assert torch.equal(R.bits(out), R.bits(out2)), f"{case.name}: the fused norm changes bits on exact inputs"
    print(f"gemv_mb {family}/{epi}: worst err / bound {worst[0]:.3f}")


@pytest.mark.parametrize("family", ["exact", "kprobe", "scaled"])
def test_gemv_mb_eight_k_slices_on_a_nan_workspace(family):
    o = ops()
    M, N, K = 32, 64, 18944
    for epi in ("plain", "bias_res"):
        case, ref = built(family, M, N, K, epi)
        ws = torch.full((o.mb_workspace_floats(N, K) + 1024,), float("nan"), dtype=torch.float32, device=DEV)
        outs = [R.run_dense(o.gemv_mb, case, DEV, workspace=ws) for _ in range(2)]
        q = R.assert_case(case, outs[0], ref, what="gemv_mb K slices")
        assert torch.equal(R.bits(outs[0]), R.bits(outs[1]))
        print(f"gemv_mb 8 slices {family}/{epi}: " + ("exact" if case.exact else f"err / bound {q:.3f}"))


ROUTES = {1: "gemv", 2: "gemv_mb", 32: "gemv_mb", 33: "gemm_skinny", 64: "gemm_skinny", 65: "bagel_gemm_bf16_ws"}


@pytest.mark.parametrize("family", ["exact", "roundpoint", "scaled"])
def test_gemm_routing(family, monkeypatch):
    """ops.gemm(variant=None): gemv (1 row), gemv_mb (2 .. 32), skinny (33 .. 64), the tile kernel (65).  The route each call takes is
    recorded and asserted, so an environment (BAGEL_GEMV_MB, BAGEL_GEMV_MB_ROWS, BAGEL_GEMM_VARIANT) or a routing change that sends a
    row count elsewhere fails here and does not pass on another path's results."""
    o, worst, taken = ops(), 0.0, []

    def spy(name):
        inner = getattr(o, name)

        def f(*a, **k):
            taken.append(name)
            return inner(*a, **k)
        return f
    for name in ("gemv", "gemv_mb", "gemm_skinny"):
        monkeypatch.setattr(o, name, spy(name))
    for M in (1, 2, 32, 33, 64, 65):
        for epi in ("plain", "bias_res", "swiglu"):
            case, ref = built(family, M, 160, 704, epi)
            del taken[:]
            out = R.run_gemm(o, case, R.gemm_args(case, DEV), None)
            assert taken == ([ROUTES[M]] if M < 65 else []), f"{case.name}: routed through {taken or 'the tile GEMM'}, expected {ROUTES[M]}"
            worst = max(worst, R.assert_case(case, out, ref, what=f"routed M = {M} ({ROUTES[M]})"))
    print(f"routing {family}: " + ("exact (SwiGLU: within one element-ulp)" if family in R.EXACT_FAMILIES else f"worst err / bound {worst:.3f}"))


# ------------------------------------------------------------------------------------------------------------
# fp8 persistent kernel
# ------------------------------------------------------------------------------------------------------------
def e4m3_codes(x):
    """fp32 values in {-1, 0, +1} -> OCP e4m3 bytes."""
    c = torch.zeros(x.shape, dtype=torch.uint8)
    c[x == 1], c[x == -1] = 0x38, 0xB8
    return c


@pytest.mark.parametrize("epi", ["plain", "bias", "res", "swiglu"])
@pytest.mark.parametrize("layout", ["exact", "edges"])
def test_gemm_fp8_exact(epi, layout):
    """Codes +-1 / 0 with power-of-two scales: (sa sw) acc is exact in fp32, so the fp8 kernel must give the bits of the float64 rounding
    sequence; SwiGLU: the bits of the bf16 tile kernel on the equivalent operands (one silu_f on one input).  A row list names the rows;
    ``edges``: the rows it does not name hold NaN codes, C rows and columns outside it sentinels."""
    o = ops()
    for M, N, K in [(300, 288, 256), (1100, 544, 1152)]:
        p, sa, sw = R.fp8_exact(M, N, K, seed=3)
        pad = layout == "edges"
        rows = [2 * i + 1 for i in range(M)] if pad else list(range(M))
        Mp = 2 * M + 3 if pad else M
        e = {"swiglu": R.EPI_SWIGLU}.get(epi, R.EPI_NONE)
        Nout = N // 2 if e else N
        ldc = Nout + 8 if pad else Nout
        Aeff = torch.full((Mp, K), float("nan"), dtype=BF16)
        Aeff[rows] = (p["A"].float() * sa[:, None]).to(BF16)
        C0 = torch.full((Mp, ldc), R.SENTINEL, dtype=BF16)
        C0[rows, :Nout] = p["R"][:, :Nout] if epi == "res" else torch.full((M, Nout), float("nan"), dtype=BF16)
        case = R.Case(f"fp8 {layout}/{epi} {M}x{N}x{K}", Aeff, [dict(W=(p["W"].float() * sw[:, None]).to(BF16), bias=p["bias"] if epi == "bias" else None,
                                                                   a_rows=rows, c_rows=rows, M=M)], epi=e, res=epi == "res", C0=C0, exact=True)
        Aq = torch.full((Mp, K), 0x7F, dtype=torch.uint8)         # NaN codes
        Aq[rows] = e4m3_codes(p["A"].float())
        sap = torch.full((Mp,), float("nan"))
        sap[rows] = sa
        C = C0.to(DEV).clone()
        Cv = C[:, :Nout]
        o.gemm_fp8(Aq.to(DEV), sap.to(DEV), e4m3_codes(p["W"].float()).to(DEV), sw.to(DEV), Cv, bias=case.groups[0]["bias"].to(DEV) if epi == "bias" else None,
                   rows=torch.tensor(rows, dtype=torch.int32, device=DEV), M=M, residual=Cv if epi == "res" else None, epilogue=e)
        got = C.cpu()
        R.assert_case(case, got, what="gemm_fp8")
        if e:
            same = R.run_gemm(o, case, R.gemm_args(case, DEV), 0)
            assert torch.equal(R.bits(got), R.bits(same)), f"{case.name}: the fp8 kernel differs from the bf16 tile kernel on exact inputs"
