"""GPU parity of the batched-decode weight stream on MXFP4 weights (bagel_gemv_mb_w4_bf16, csrc/gemv_mb_w4.hip: 1..32 e4m3 activation rows with row scales x
the stored codes on the block-scaled MFMA) against the CPU restatement oracle/mxfp4.py::gemv_w4.

  1. designed inputs on which every fp32 partial sum is exact (any summation order gives the float64 product): scale-byte routing, fragment layout,
     request <-> lane mapping, K partition, K slices and tails are checked with ``torch.equal``.  That rests on the block-scaled MFMA adding exactly
     representable partial sums exactly, which the unchanged ``ops.gemv_w4`` is asked first on rows 0-3 of each case: exact there -> the new kernel must be
     too; otherwise both are held to ``close(ulps=2)`` and the test prints that it fell back;
  2. random inputs against the restatement (which does norm and quantisation; the device side is rmsnorm_fp8 / quantize_rows_fp8 + the stream);
  3. request isolation: other rows' data never reaches a row's output bits;
  4. the 7B projection shapes against the large-M kernel (ops.gemm_w4, pinned to the oracle in tests/test_gemm_w4_gpu.py) on the same quantised rows:
     the same sums in another order, 2 bf16 ulp as tests/test_gemv_mb_gpu.py / tests/test_mxfp4_gpu.py give a re-ordered fp32 accumulation;
  5. refusals: argument errors that name the argument, nothing launched."""
import functools

import pytest
import torch

from oracle import mxfp4 as MX
from tests.test_ops_gpu import BF16, DEV, close, ops

pytestmark = pytest.mark.gpu

E2M1_MAGS = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


# ------------------------------------------------------------------------------------------------------------
# 1. designed exact inputs
# ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def designed(M, N, K):
    """-> x [M, K] (integers in [-3, 3], one 448 per row: sa == 1, codes == values), W [N, K] (E2M1 magnitude x random sign x 2^e, e = (5 n + 3 kblock) % 5 - 2,
    one element per block pinned to +-4 / +-6 so the quantiser finds exactly e), small-integer bias [N] and residual [M, N]."""
    g = torch.Generator().manual_seed(1000 * M + N + K)
    nb = K // 32
    mag = E2M1_MAGS[torch.randint(0, 8, (N, nb, 32), generator=g)]
    pin = torch.randint(0, 32, (N, nb), generator=g)
    mag.scatter_(2, pin[:, :, None], torch.where(torch.rand(N, nb, 1, generator=g) < 0.5, 4.0, 6.0))
    sign = torch.where(torch.rand(N, nb, 32, generator=g) < 0.5, -1.0, 1.0)
    e = (5 * torch.arange(N)[:, None] + 3 * torch.arange(nb)[None, :]) % 5 - 2
    W = (mag * sign * torch.pow(2.0, e.float())[:, :, None]).view(N, K).to(BF16)
    x = torch.randint(-3, 4, (M, K), generator=g).float()
    x[torch.arange(M), torch.randint(0, K, (M,), generator=g)] = 448.0
    bias = torch.randint(-8, 9, (N,), generator=g).float().to(BF16)
    R = torch.randint(-8, 9, (M, N), generator=g).float().to(BF16)
    # the construction is what it claims to be
    q, sb = MX.quantize_mxfp4(W)
    assert torch.equal(MX.dequant_mxfp4(q, sb), W.float()) and torch.equal(sb.int() - 127, e.int())
    return x.to(BF16), W, bias, R, e


def exact_ref(x, W, bias=None, R=None):
    acc = x.double() @ W.double().t()                               # every partial sum: a multiple of 2^-3 below 2^21 -- exact in fp32 in any order
    assert acc.abs().max() < 2 ** 21
    if bias is not None:
        acc = acc + bias.double()
    c = acc.float().to(BF16)
    return c if R is None else (c.float() + R.float()).to(BF16)


def run_stream(o, x, q, s, mode, bias, R, rows_extra=0, norm_w=None):
    """quantiser launch + gemv_mb_w4 on device tensors -> C [M + rows_extra, Nout] (NaN-filled first; residual mode: in place on the R rows)."""
    M, N = x.shape[0], q.shape[0]
    swiglu = mode.endswith("swiglu")
    Nout = N // 2 if swiglu else N
    C = torch.full((M + rows_extra, Nout), float("nan"), dtype=BF16, device=DEV)
    if mode == "residual":
        C[:M] = R.to(DEV)
    xd = x.to(DEV)
    if norm_w is not None:
        aq, sa = torch.empty(x.shape, dtype=torch.uint8, device=DEV), torch.empty((M,), dtype=torch.float32, device=DEV)
        o.rmsnorm_fp8(xd, norm_w.to(DEV), aq, sa, 1e-6)
    else:
        aq, sa = o.quantize_rows_fp8(xd)
    ws = torch.full((o.mb_w4_workspace_floats(N, x.shape[1]) + 1024,), float("nan"), dtype=torch.float32, device=DEV)
    o.gemv_mb_w4(aq, sa, q, s, C, bias=bias.to(DEV) if mode == "bias" else None, residual=C if mode == "residual" else None,
                 epilogue=o.EPI_SWIGLU16 if swiglu else o.EPI_NONE, M=M, workspace=ws)
    torch.cuda.synchronize()
    return C, sa


DESIGNED_SHAPES = [(5, 48, 128), (17, 64, 640), (32, 64, 3584), (20, 32, 18944)]


@pytest.mark.parametrize("mode", ["plain", "bias", "residual"])
@pytest.mark.parametrize("M,N,K", DESIGNED_SHAPES)
def test_designed_inputs_bit_for_bit(M, N, K, mode):
    o = ops()
    x, W, bias, R, e = designed(M, N, K)
    q, s = o.quantize_rows_mxfp4(W.to(DEV))
    qr, sr = MX.quantize_mxfp4(W)
    assert torch.equal(q.cpu(), qr) and torch.equal(s.cpu(), MX.permute_scales(sr))
    b = bias if mode == "bias" else None
    r = R if mode == "residual" else None
    ref = exact_ref(x, W, b, r)
    # the yardstick: the parent's kernel on rows 0-3 (it quantises the rows itself)
    P = R[:4].to(DEV).clone() if r is not None else torch.full((4, N), float("nan"), dtype=BF16, device=DEV)
    o.gemv_w4(x[:4].to(DEV), q, s, P, bias=None if b is None else b.to(DEV), residual=P if r is not None else None)
    C, sa = run_stream(o, x, q, s, mode, bias, R, rows_extra=2)
    assert torch.equal(sa.cpu(), torch.ones(M)), "the designed rows quantise with a scale of exactly 1"
    assert torch.isnan(C[M:]).all(), "rows >= M were written"
    if torch.equal(P.cpu(), ref[:4]):
        bad = (C[:M].cpu() != ref).nonzero()
        assert torch.equal(C[:M].cpu(), ref), f"{len(bad)} of {ref.numel()} elements differ from the float64 product, first (m, n) = {bad[0].tolist()}"
    else:
        print(f"designed {M}x{N}x{K} {mode}: ops.gemv_w4 is NOT bit-equal to the float64 product on these inputs -- falling back to close(ulps=2) for both kernels")
        full = MX.gemv_w4(x, qr, sr, bias=b, residual=r)
        close(P.cpu(), full[:4], ulps=2, what="gemv_w4 on designed inputs")
        close(C[:M].cpu(), full, ulps=2, what="gemv_mb_w4 on designed inputs")


def test_designed_inputs_swiglu():
    """g and u bit for bit through a plain run of the same weights; the fused result within one bf16 ulp of silu(g) * u (one silu_f on one input, as
    tests/test_gemm_designed_gpu.py holds its SwiGLU cases)."""
    o = ops()
    M, N, K = 17, 64, 640
    x, W, bias, R, e = designed(M, N, K)
    q, s = o.quantize_rows_mxfp4(W.to(DEV))
    plain, _ = run_stream(o, x, q, s, "plain", bias, R)
    ref = exact_ref(x, W)
    P = torch.full((4, N), float("nan"), dtype=BF16, device=DEV)
    o.gemv_w4(x[:4].to(DEV), q, s, P)
    if torch.equal(P.cpu(), ref[:4]):
        assert torch.equal(plain.cpu(), ref)
    else:
        print("designed swiglu: ops.gemv_w4 is NOT bit-equal to the float64 product on these inputs -- falling back to close(ulps=2)")
        close(plain.cpu(), MX.gemv_w4(x, *MX.quantize_mxfp4(W)), ulps=2, what="gemv_mb_w4 plain on designed inputs")
    gu = plain.cpu().view(M, N // 32, 2, 16)
    gt, up = gu[:, :, 0].reshape(M, -1), gu[:, :, 1].reshape(M, -1)
    fused, _ = run_stream(o, x, q, s, "swiglu", bias, R)
    want = (torch.nn.functional.silu(gt.double()).float().to(BF16).double() * up.double())
    ulp = torch.pow(2.0, torch.floor(torch.log2(want.abs().clamp_min(1e-30))) - 7)       # one bf16 ulp of each element
    d = (fused.cpu().double() - want).abs()
    assert torch.isfinite(fused).all() and (d <= ulp).all(), f"fused SwiGLU: worst error {(d / ulp).max().item():.3f} element-ulps"


# ------------------------------------------------------------------------------------------------------------
# 2. random inputs against the restatement
# ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(M, N, K):
    g = torch.Generator().manual_seed(N + K + M)
    x = (torch.randn(M, K, generator=g) * 1.5).to(BF16)
    W = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF16)
    bias = (torch.randn(N, generator=g) * 0.1).to(BF16)
    nw = (1.0 + 0.1 * torch.randn(K, generator=g)).to(BF16)
    R = torch.randn(M, N, generator=g).to(BF16)
    qr, sr = MX.quantize_mxfp4(W)
    return x, W, bias, nw, R, qr, sr


@pytest.mark.parametrize("mode", ["plain", "bias", "residual", "swiglu", "norm", "norm_swiglu"])
@pytest.mark.parametrize("M,N,K", [(5, 64, 128), (16, 96, 640), (17, 160, 3584), (32, 64, 18944), (32, 4608, 3584)])
def test_gemv_mb_w4_matches_restatement(M, N, K, mode):
    o = ops()
    x, W, bias, nw, R, qr, sr = random_case(M, N, K)
    q, s = o.quantize_rows_mxfp4(W.to(DEV))
    assert torch.equal(q.cpu(), qr) and torch.equal(s.cpu(), MX.permute_scales(sr))
    swiglu = mode.endswith("swiglu")
    norm_w = nw if mode.startswith("norm") else None
    C, _ = run_stream(o, x, q, s, mode, bias, R, rows_extra=3, norm_w=norm_w)
    ref = MX.gemv_w4(x, qr, sr, bias=bias if mode == "bias" else None, residual=R if mode == "residual" else None, swiglu=swiglu, norm_w=norm_w, eps=1e-6)
    assert torch.isnan(C[M:]).all(), "rows >= M were written"
    close(C[:M].cpu(), ref, ulps=2, what=f"gemv_mb_w4 {mode} M={M} N={N} K={K}")


# ------------------------------------------------------------------------------------------------------------
# 3. request isolation
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3584, 18944])
def test_request_isolation(K):
    o = ops()
    M, N = 32, 64
    x, W, bias, nw, R, qr, sr = random_case(M, N, K)
    q, s = o.quantize_rows_mxfp4(W.to(DEV))
    a, _ = run_stream(o, x, q, s, "plain", bias, R)
    y = x.clone()
    y[1::2] = (torch.randn(M // 2, K, generator=torch.Generator().manual_seed(7)) * 40.0).to(BF16)      # other data, other row scales
    b, _ = run_stream(o, y, q, s, "plain", bias, R)
    assert torch.equal(a[0::2].view(torch.int16), b[0::2].view(torch.int16)), "a row's output depends on the other requests' data"
    assert not torch.equal(a[1::2], b[1::2])


# ------------------------------------------------------------------------------------------------------------
# 4. the 7B projection shapes against the large-M kernel
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,swiglu", [(4608, 3584, False), (3584, 3584, False), (37888, 3584, True), (3584, 18944, False)])
def test_agrees_with_gemm_w4_at_7b_shapes(N, K, swiglu):
    o = ops()
    M = 32
    g = torch.Generator(device=DEV).manual_seed(N + K)
    x = (torch.randn(M, K, generator=g, device=DEV) * 1.5).to(BF16)
    q, s = o.quantize_rows_mxfp4((torch.randn(N, K, generator=g, device=DEV) * K ** -0.5).to(BF16))
    aq, sa = o.quantize_rows_fp8(x)
    epi = o.EPI_SWIGLU16 if swiglu else o.EPI_NONE
    Nout = N // 2 if swiglu else N
    R = None if swiglu else torch.randn(M, N, generator=g, device=DEV).to(BF16)
    Cs = torch.full((M, Nout), float("nan"), dtype=BF16, device=DEV)
    Cg = torch.full((M, Nout), float("nan"), dtype=BF16, device=DEV)
    o.gemv_mb_w4(aq, sa, q, s, Cs, residual=R, epilogue=epi)
    o.gemm_w4(aq, sa, q, s, Cg, residual=R, epilogue=epi)
    torch.cuda.synchronize()
    close(Cs, Cg, ulps=2, what=f"gemv_mb_w4 vs gemm_w4 N={N} K={K}")
    again = torch.full((M, Nout), float("nan"), dtype=BF16, device=DEV)
    o.gemv_mb_w4(aq, sa, q, s, again, residual=R, epilogue=epi)
    assert torch.equal(Cs.view(torch.int16), again.view(torch.int16)), "two launches on the same operands differ: the summation order is not fixed"


# ------------------------------------------------------------------------------------------------------------
# 5. refusals
# ------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_launch_nothing():
    from bagel_amd import _lib
    o = ops()
    L = _lib.lib()
    u8 = lambda *sh: torch.zeros(sh, dtype=torch.uint8, device=DEV)  # noqa: E731
    sa = torch.ones(64, dtype=torch.float32, device=DEV)
    bias = torch.zeros(64, dtype=BF16, device=DEV)

    def call(M, N, K, epi=0, bias=None, rows=40):
        aq, wq, ws = u8(rows, K), u8(N, K // 2), u8(N, ((K // 128 + 3) // 4) * 16)
        C = torch.full((rows, N), float("nan"), dtype=BF16, device=DEV)
        rc = L.bagel_gemv_mb_w4_bf16(aq.data_ptr(), aq.stride(0), sa.data_ptr(), wq.data_ptr(), wq.stride(0), ws.data_ptr(), ws.stride(0),
                                     None if bias is None else bias.data_ptr(), None, 0, C.data_ptr(), C.stride(0), M, N, K, epi, None, 0,
                                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.isnan(C).all(), "a refused call wrote to C"
        return rc, L.bagel_hip_last_error().decode()
    rc, msg = call(0, 64, 256)
    assert rc == -1 and "M=0" in msg, (rc, msg)
    rc, msg = call(33, 64, 256)
    assert rc == -1 and "M=33" in msg, (rc, msg)
    rc, msg = call(8, 64, 192)
    assert rc == -1 and "K=192" in msg, (rc, msg)
    rc, msg = call(8, 64, 256, epi=o.EPI_SWIGLU16, bias=bias)
    assert rc == -1 and "SwiGLU16" in msg and "bias" in msg, (rc, msg)
    with pytest.raises(o.BagelHipError, match="M=33"):
        o.gemv_mb_w4(u8(40, 256), sa, u8(64, 128), u8(64, 16), torch.empty((40, 64), dtype=BF16, device=DEV), M=33)
    assert not o.gemv_mb_w4_supported(u8(40, 256), u8(64, 128), u8(64, 16), torch.empty((40, 64), dtype=BF16, device=DEV), None, None, o.EPI_NONE, M=33)
