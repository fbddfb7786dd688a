"""GPU parity of the batched-decode weight stream on NF4 weights (bagel_gemv_mb_nf4_bf16, csrc/gemv_mb_nf4.hip: 1..32 bf16 activation rows x the stored codes,
de-quantised in registers to bf16(code_book[code] * absmax) and multiplied on the bf16 MFMA) against the CPU restatement oracle/nf4.py.

  1. selector rows: an activation row with ONE non-zero element +-2^j reads one column of the de-quantised weight, so C[m, :] must be bf16(x * w'[:, k_m]) bit
     for bit in any summation order -- nibble order, lane <-> k mapping, absmax halves, wave ranges, slice seams and the row's end are checked with ``torch.equal``;
  2. designed inputs on which every fp32 partial sum is exact (weights in {-a, 0, +a}, a = 2^e per block; integer activations): ``torch.equal`` against the
     float64 product.  That rests on the bf16 MFMA adding exactly representable partial sums exactly, which the unchanged ``ops.gemv_mb`` on ``ops.dequantize_nf4``
     of the same codes is asked first: exact there -> the new kernel must be too; otherwise both are held to ``close(ulps=2)`` and the test prints that it fell back;
  3. random inputs against ``ops.gemv_mb`` on the de-quantised bf16 weight (same values, another order) and against oracle/nf4.py::linear_nf4 on the CPU;
  4. request isolation: other rows' data never reaches a row's output bits;
  5. the 7B projection shapes against ``ops.gemv_mb`` on the de-quantised weight;
  6. refusals: argument errors that name the argument, nothing written."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import nf4 as NF
from tests.test_ops_gpu import BF16, DEV, close, ops, ref_gemm

pytestmark = pytest.mark.gpu

SHAPES = [(5, 48, 128), (17, 64, 640), (32, 64, 3584), (20, 32, 18944)]


def epilogue_ref(acc32, bias=None, R=None):
    """mb_epilogue's rounding points on an fp32 accumulator: fp32 bias add, bf16 rounding, fp32 residual add, bf16 rounding."""
    if bias is not None:
        acc32 = acc32 + bias.float()
    c = acc32.to(BF16)
    return c if R is None else (c.float() + R.float()).to(BF16)


def run_stream(o, x, q, a, mode, bias=None, R=None, rows_extra=0):
    """gemv_mb_nf4 on device tensors -> C [M + rows_extra, Nout] (NaN-filled first; residual mode: in place on the R rows); NaN-filled, over-allocated workspace."""
    M, K, N = x.shape[0], x.shape[1], q.shape[0]
    swiglu = mode == "swiglu"
    C = torch.full((M + rows_extra, N // 2 if swiglu else N), float("nan"), dtype=BF16, device=DEV)
    if mode == "residual":
        C[:M] = R.to(DEV)
    ws = torch.full((o.mb_nf4_workspace_floats(N, K) + 1024,), float("nan"), dtype=torch.float32, device=DEV)
    o.gemv_mb_nf4(x.to(DEV), q, a, C, bias=bias.to(DEV) if mode == "bias" else None, residual=C if mode == "residual" else None,
                  epilogue=o.EPI_SWIGLU16 if swiglu else o.EPI_NONE, M=M, workspace=ws)
    torch.cuda.synchronize()
    return C


def geometry(M, N, K, epi=0):
    """(k-groups per wave, per slice, slices, workgroups per slice) as the launcher plans this shape on this device."""
    from bagel_amd import _lib
    g = (ctypes.c_int32 * 4)()
    p = ctypes.addressof(g)
    wgs = torch.cuda.get_device_properties(0).multi_processor_count
    assert _lib.lib().bagel_gemv_mb_nf4_geometry(M, N, K, epi, wgs, p, p + 4, p + 8, p + 12) == 0
    return tuple(g)


# ------------------------------------------------------------------------------------------------------------
# 1. selector rows
# ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_weight(N, K):
    g = torch.Generator().manual_seed(N + K)
    W = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF16)
    qr, ar = NF.quantize_nf4(W)
    return W, qr, ar, NF.dequantize_nf4(qr, ar)


def selector_positions(M, N, K):
    """The k positions a wrong index would show at: both nibbles of a byte and the first / last weight of every wave's group range (so: every slice seam and the
    row's end), the first and last weight of every lane's 32 and both halves of an absmax block in the row's first and last group."""
    per, sg, ks, _ = geometry(M, N, K)
    G = K // 128
    pos = {0, 1, K - 2, K - 1}
    for s in range(ks):
        for w in range(8):
            lo = s * sg + w * per
            hi = min(lo + per, (s + 1) * sg, G)
            if lo < hi:
                pos |= {128 * lo, 128 * lo + 1, 128 * hi - 2, 128 * hi - 1}
    for g in (0, G - 1):
        for q in range(4):
            pos |= {128 * g + 32 * q, 128 * g + 32 * q + 1, 128 * g + 32 * q + 30, 128 * g + 32 * q + 31}
    return sorted(pos)


@pytest.mark.parametrize("mode", ["plain", "bias", "residual"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_selector_rows_bit_for_bit(M, N, K, mode):
    o = ops()
    W, qr, ar, Wd = random_weight(N, K)
    q, a = o.quantize_nf4(W.to(DEV))
    assert torch.equal(q.cpu(), qr) and torch.equal(a.cpu(), ar)
    g = torch.Generator().manual_seed(K + M)
    bias = (torch.randn(N, generator=g) * 0.1).to(BF16)
    R = torch.randn(M, N, generator=g).to(BF16)
    pos = selector_positions(M, N, K)
    for c0 in range(0, len(pos), M):
        kk = (pos[c0:c0 + M] * M)[:M]                                # (the last chunk repeats its positions: every row is a selector row)
        idx = torch.arange(c0, c0 + M)
        v = torch.where(idx % 2 == 1, -1.0, 1.0) * torch.pow(2.0, (idx % 5 - 2).float())
        x = torch.zeros(M, K)
        x[torch.arange(M), torch.tensor(kk)] = v
        ref = epilogue_ref(v[:, None] * Wd[:, kk].t().float(), bias if mode == "bias" else None, R if mode == "residual" else None)   # the product is exact
        C = run_stream(o, x.to(BF16), q, a, mode, bias, R, rows_extra=2)
        assert torch.isnan(C[M:]).all(), "rows >= M were written"
        got = C[:M].cpu()
        if not torch.equal(got, ref):
            bad = (got != ref).nonzero()
            m, n = bad[0].tolist()
            raise AssertionError(f"{len(bad)} of {ref.numel()} elements differ; first: row {m} (k = {kk[m]}, x = {v[m].item()}), n = {n}: got {got[m, n].item()} "
                                 f"want {ref[m, n].item()}")


# ------------------------------------------------------------------------------------------------------------
# 2. designed exact accumulation
# ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def designed(M, N, K):
    """-> x [M, K] (integers in [-3, 3]), W [N, K] in {-a, 0, +a} with a = 2^e per 64-block, e = (5 n + 3 block) % 5 - 2, one element per block pinned to +-a (so
    the quantiser finds exactly codes 0 / 7 / 15 and absmax = a), small-integer bias [N] and residual [M, N]."""
    g = torch.Generator().manual_seed(1000 * M + N + K)
    nb = K // 64
    t = torch.randint(-1, 2, (N, nb, 64), generator=g).float()
    pin = torch.randint(0, 64, (N, nb), generator=g)
    t.scatter_(2, pin[:, :, None], torch.where(torch.rand(N, nb, 1, generator=g) < 0.5, -1.0, 1.0))
    e = (5 * torch.arange(N)[:, None] + 3 * torch.arange(nb)[None, :]) % 5 - 2
    amax = torch.pow(2.0, e.float())
    W = (t * amax[:, :, None]).view(N, K).to(BF16)
    x = torch.randint(-3, 4, (M, K), generator=g).float().to(BF16)
    bias = torch.randint(-8, 9, (N,), generator=g).float().to(BF16)
    R = torch.randint(-8, 9, (M, N), generator=g).float().to(BF16)
    # the construction is what it claims to be
    qr, ar = NF.quantize_nf4(W)
    codes = NF.codes_of(qr)
    assert torch.equal(ar, amax) and set(codes.unique().tolist()) <= {0, 7, 15}
    assert torch.equal(codes.view(N, nb, 64), (t * 7.5 + 7.5).long().clamp(0, 15)) and torch.equal(NF.dequantize_nf4(qr, ar), W)
    return x, W, bias, R, qr, ar


def exact_ref(x, W, bias=None, R=None):
    acc = x.double() @ W.double().t()                               # every partial sum: a multiple of 2^-2 below 2^22 -- exact in fp32 in any order
    assert acc.abs().max() < 2 ** 21
    if bias is not None:
        acc = acc + bias.double()
    c = acc.float().to(BF16)
    return c if R is None else (c.float() + R.float()).to(BF16)


def yardstick(o, x, q, a, mode, bias, R):
    """The unchanged bf16 stream (ops.gemv_mb) on ops.dequantize_nf4 of the same codes."""
    M, N = x.shape[0], q.shape[0]
    P = R.to(DEV).clone() if mode == "residual" else torch.full((M, N), float("nan"), dtype=BF16, device=DEV)
    o.gemv_mb(x.to(DEV), o.dequantize_nf4(q, a).contiguous(), P, bias=bias.to(DEV) if mode == "bias" else None, residual=P if mode == "residual" else None, M=M)
    torch.cuda.synchronize()
    return P.cpu()


@pytest.mark.parametrize("mode", ["plain", "bias", "residual"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_designed_inputs_bit_for_bit(M, N, K, mode):
    o = ops()
    x, W, bias, R, qr, ar = designed(M, N, K)
    q, a = o.quantize_nf4(W.to(DEV))
    assert torch.equal(q.cpu(), qr) and torch.equal(a.cpu(), ar)
    b = bias if mode == "bias" else None
    r = R if mode == "residual" else None
    ref = exact_ref(x, W, b, r)
    P = yardstick(o, x, q, a, mode, bias, R)
    C = run_stream(o, x, q, a, mode, bias, R, rows_extra=2)
    assert torch.isnan(C[M:]).all(), "rows >= M were written"
    if torch.equal(P, ref):
        bad = (C[:M].cpu() != ref).nonzero()
        assert torch.equal(C[:M].cpu(), ref), f"{len(bad)} of {ref.numel()} elements differ from the float64 product, first (m, n) = {bad[0].tolist()}"
    else:
        print(f"designed {M}x{N}x{K} {mode}: ops.gemv_mb is NOT bit-equal to the float64 product on these inputs -- falling back to close(ulps=2) for both kernels")
        close(P, ref, ulps=2, what="gemv_mb on designed inputs")
        close(C[:M].cpu(), ref, ulps=2, what="gemv_mb_nf4 on designed inputs")


def test_designed_inputs_swiglu():
    """g and u bit for bit through a plain run of the same weights; the fused result within one bf16 ulp of silu(g) * u (one silu_f on one input, as
    tests/test_gemm_designed_gpu.py holds its SwiGLU cases)."""
    o = ops()
    M, N, K = 17, 64, 640
    x, W, bias, R, qr, ar = designed(M, N, K)
    q, a = o.quantize_nf4(W.to(DEV))
    plain = run_stream(o, x, q, a, "plain")
    ref = exact_ref(x, W)
    if torch.equal(yardstick(o, x, q, a, "plain", bias, R), ref):
        assert torch.equal(plain.cpu(), ref)
    else:
        print("designed swiglu: ops.gemv_mb is NOT bit-equal to the float64 product on these inputs -- falling back to close(ulps=2)")
        close(plain.cpu(), ref, ulps=2, what="gemv_mb_nf4 plain on designed inputs")
    gu = plain.cpu().view(M, N // 32, 2, 16)
    gt, up = gu[:, :, 0].reshape(M, -1), gu[:, :, 1].reshape(M, -1)
    fused = run_stream(o, x, q, a, "swiglu")
    want = (F.silu(gt.double()).float().to(BF16).double() * up.double())
    ulp = torch.pow(2.0, torch.floor(torch.log2(want.abs().clamp_min(1e-30))) - 7)       # one bf16 ulp of each element
    d = (fused.cpu().double() - want).abs()
    assert torch.isfinite(fused).all() and (d <= ulp).all(), f"fused SwiGLU: worst error {(d / ulp).max().item():.3f} element-ulps"


# ------------------------------------------------------------------------------------------------------------
# 3. random inputs
# ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(M, N, K):
    W, qr, ar, Wd = random_weight(N, K)
    g = torch.Generator().manual_seed(N + K + M)
    x = (torch.randn(M, K, generator=g) * 1.5).to(BF16)
    bias = (torch.randn(N, generator=g) * 0.1).to(BF16)
    R = torch.randn(M, N, generator=g).to(BF16)
    return x, W, bias, R, qr, ar, Wd


@pytest.mark.parametrize("M,N,K,mode", [(5, 512, 512, "plain"), (16, 1024, 512, "swiglu"), (32, 512, 1024, "residual"), (9, 48, 128, "bias")])
def test_random_inputs_match_bf16_stream_and_restatement(M, N, K, mode):
    o = ops()
    x, W, bias, R, qr, ar, Wd = random_case(M, N, K)
    q, a = o.quantize_nf4(W.to(DEV))
    assert torch.equal(q.cpu(), qr) and torch.equal(a.cpu(), ar)
    swiglu = mode == "swiglu"
    C = run_stream(o, x, q, a, mode, bias, R, rows_extra=3)
    assert torch.isnan(C[M:]).all(), "rows >= M were written"
    # the bf16 stream on the de-quantised weight: the same values in another order
    Nout = N // 2 if swiglu else N
    P = R.to(DEV).clone() if mode == "residual" else torch.full((M, Nout), float("nan"), dtype=BF16, device=DEV)
    wd = o.dequantize_nf4(q, a).contiguous()
    assert torch.equal(wd.cpu().view(torch.int16), Wd.view(torch.int16))
    o.gemv_mb(x.to(DEV), wd, P, bias=bias.to(DEV) if mode == "bias" else None, residual=P if mode == "residual" else None,
              epilogue=o.EPI_SWIGLU16 if swiglu else o.EPI_NONE, M=M)
    budget = 8e-3 if swiglu else 4e-3                                # tests/test_nf4_gpu.py: two chained roundings / one
    close(C[:M], P, ulps=2, rel_l2=budget, what=f"gemv_mb_nf4 vs gemv_mb on the de-quantised weight, {mode} M={M} N={N} K={K}")
    # the restatement: Linear4bit with bf16 compute, then the epilogue on its bf16 output
    y = NF.linear_nf4(x, qr, ar, bias if mode == "bias" else None)
    if swiglu:
        gu = y.view(M, N // 32, 2, 16)
        y = F.silu(gu[:, :, 0].reshape(M, -1)) * gu[:, :, 1].reshape(M, -1)
    elif mode == "residual":
        y = R + y
    close(C[:M].cpu(), y, ulps=2, rel_l2=budget, what=f"gemv_mb_nf4 vs linear_nf4, {mode} M={M} N={N} K={K}")
    close(C[:M].cpu(), ref_gemm(x, Wd, bias if mode == "bias" else None, 3 if swiglu else 0, R if mode == "residual" else None), ulps=2, rel_l2=budget,
          what=f"gemv_mb_nf4 vs the fp32 product on the de-quantised weight, {mode}")


# ------------------------------------------------------------------------------------------------------------
# 4. request isolation
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(7, 48, 640), (23, 32, 18944)])
def test_request_isolation(M, N, K):
    o = ops()
    x, W, bias, R, qr, ar, Wd = random_case(M, N, K)
    q, a = o.quantize_nf4(W.to(DEV))
    keep = M // 2
    A = run_stream(o, x, q, a, "plain")
    y = (torch.randn(M, K, generator=torch.Generator().manual_seed(7)) * 40.0).to(BF16)      # other data in every other row
    y[keep] = x[keep]
    B = run_stream(o, y, q, a, "plain")
    assert torch.equal(A[keep].view(torch.int16), B[keep].view(torch.int16)), "a row's output depends on the other requests' data"
    others = [m for m in range(M) if m != keep]
    assert not torch.equal(A[others], B[others])


# ------------------------------------------------------------------------------------------------------------
# 5. the 7B projection shapes
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,mode", [(16, 4608, 3584, "bias"), (32, 37888, 3584, "swiglu"), (20, 3584, 3584, "residual"), (32, 3584, 18944, "residual")])
def test_agrees_with_bf16_stream_at_7b_shapes(M, N, K, mode):
    o = ops()
    g = torch.Generator(device=DEV).manual_seed(N + K)
    x = (torch.randn(M, K, generator=g, device=DEV) * 1.5).to(BF16)
    q, a = o.quantize_nf4((torch.randn(N, K, generator=g, device=DEV) * K ** -0.5).to(BF16))
    wd = o.dequantize_nf4(q, a).contiguous()
    swiglu = mode == "swiglu"
    epi = o.EPI_SWIGLU16 if swiglu else o.EPI_NONE
    Nout = N // 2 if swiglu else N
    bias = (torch.randn(N, generator=g, device=DEV) * 0.1).to(BF16) if mode == "bias" else None
    R = torch.randn(M, N, generator=g, device=DEV).to(BF16) if mode == "residual" else None
    Cs = torch.full((M, Nout), float("nan"), dtype=BF16, device=DEV)
    Cg = torch.full((M, Nout), float("nan"), dtype=BF16, device=DEV)
    o.gemv_mb_nf4(x, q, a, Cs, bias=bias, residual=R, epilogue=epi)
    o.gemv_mb(x, wd, Cg, bias=bias, residual=R, epilogue=epi)
    torch.cuda.synchronize()
    close(Cs, Cg, ulps=2, rel_l2=8e-3 if swiglu else 4e-3, what=f"gemv_mb_nf4 vs gemv_mb on the de-quantised weight M={M} N={N} K={K}")
    again = torch.full((M, Nout), float("nan"), dtype=BF16, device=DEV)
    o.gemv_mb_nf4(x, q, a, again, bias=bias, residual=R, epilogue=epi)
    assert torch.equal(Cs.view(torch.int16), again.view(torch.int16)), "two launches on the same operands differ: the summation order is not fixed"


# ------------------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_write_nothing():
    from bagel_amd import _lib
    o = ops()
    L = _lib.lib()
    bias = torch.zeros(64, dtype=BF16, device=DEV)

    def call(M, N, K, epi=0, bias=None, rows=40):
        A = torch.zeros((rows, K), dtype=BF16, device=DEV)
        wq = torch.zeros((N, K // 2), dtype=torch.uint8, device=DEV)
        am = torch.ones((N, max(K // 64, 1)), dtype=torch.float32, device=DEV)
        C = torch.full((rows, N), float("nan"), dtype=BF16, device=DEV)
        rc = L.bagel_gemv_mb_nf4_bf16(A.data_ptr(), A.stride(0), wq.data_ptr(), wq.stride(0), am.data_ptr(), None if bias is None else bias.data_ptr(), None, 0,
                                      C.data_ptr(), C.stride(0), M, N, K, epi, None, 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.isnan(C).all(), "a refused call wrote to C"
        return rc, L.bagel_hip_last_error().decode()
    for (M, N, K, epi, b), words in (((0, 64, 256, 0, None), ["M=0"]), ((33, 64, 256, 0, None), ["M=33"]), ((8, 64, 192, 0, None), ["K=192"]),
                                     ((8, 40, 256, 0, None), ["N=40"]), ((8, 48, 256, 3, None), ["N=48"]), ((8, 64, 256, 3, bias), ["SwiGLU16", "bias"])):
        rc, msg = call(M, N, K, epi, b)
        assert rc == -1 and all(w in msg for w in words), (M, N, K, epi, rc, msg)
    A = torch.zeros((40, 256), dtype=BF16, device=DEV)
    wq = torch.zeros((64, 128), dtype=torch.uint8, device=DEV)
    am = torch.ones((64, 4), dtype=torch.float32, device=DEV)
    C = torch.full((40, 64), float("nan"), dtype=BF16, device=DEV)
    with pytest.raises(o.BagelHipError, match="M=33"):
        o.gemv_mb_nf4(A, wq, am, C, M=33)
    with pytest.raises(o.BagelHipError, match="absmax"):
        o.gemv_mb_nf4(A, wq, torch.ones((64, 8), dtype=torch.float32, device=DEV), C, M=8)
    with pytest.raises(o.BagelHipError, match="absmax"):
        o.gemv_mb_nf4(A, wq, torch.ones((4, 64), dtype=torch.float32, device=DEV).t(), C, M=8)
    assert not o.gemv_mb_nf4_supported(A, wq, am, C, None, None, o.EPI_NONE, M=33)
    assert not o.gemv_mb_nf4_supported(A, wq, torch.ones((64, 8), dtype=torch.float32, device=DEV), C, None, None, o.EPI_NONE, M=8)
    assert o.gemv_mb_nf4_supported(A, wq, am, C, None, None, o.EPI_NONE, M=8)
    # a sliced row with a workspace that is too small
    K = 18944
    A = torch.zeros((8, K), dtype=BF16, device=DEV)
    wq = torch.zeros((32, K // 2), dtype=torch.uint8, device=DEV)
    am = torch.ones((32, K // 64), dtype=torch.float32, device=DEV)
    C2 = torch.full((8, 32), float("nan"), dtype=BF16, device=DEV)
    with pytest.raises(o.BagelHipError, match="workspace"):
        o.gemv_mb_nf4(A, wq, am, C2, workspace=torch.zeros(16, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    assert torch.isnan(C).all() and torch.isnan(C2).all(), "a refused call wrote to C"
