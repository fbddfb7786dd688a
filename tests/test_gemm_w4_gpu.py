"""GPU parity of the large-M MXFP4 GEMM (bagel_gemm_w4_bf16: e4m3 row-quantised activations x MXFP4 weights on the block-scaled MFMA, the
product of the whole-model load mode weight_store = "mxfp4") against the CPU restatement oracle/mxfp4.py::gemv_w4, with the gate of the
small-M sibling kernel (tests/test_mxfp4_gpu.py: close(..., ulps=2)).

The restatement quantises the bf16 activation rows itself (oracle/fp8.py); the device side quantises them with bagel_quantize_rows_fp8, so a
disagreement of the two quantisers would show here as well.  For the widest N (the 7B gate/up projection) the CPU side checks a sampled set of
whole 32-row weight blocks (one gate + one up fragment each) of the full device output -- output columns are independent of each other."""
import pytest
import torch

from oracle import mxfp4 as MX
from tests.test_ops_gpu import BF16, DEV, close, ops

pytestmark = pytest.mark.gpu

MODES = ["plain", "bias", "residual", "swiglu", "rows"]
# M = 1, M off every tile edge (37, 300, 515), a tile-exact M (1024), a ragged last N tile (160), the four 7B (K, N) pairs
SHAPES = [(1, 64, 128), (37, 160, 256), (300, 160, 640), (1024, 512, 1024), (515, 4608, 3584), (300, 3584, 3584), (130, 37888, 3584),
          (300, 3584, 18944)]


def _case(M, N, K, mode, seed):
    g = torch.Generator().manual_seed(seed)
    Mtot = M + 9 if mode == "rows" else M
    x = (torch.randn(Mtot, K, generator=g) * 1.5).to(BF16)
    W = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF16)
    swiglu = mode == "swiglu" or (mode == "rows" and N == 37888)
    bias = (torch.randn(N, generator=g) * 0.1).to(BF16) if mode in ("bias", "rows") and not swiglu else None
    Nout = N // 2 if swiglu else N
    R = torch.randn(Mtot, Nout, generator=g).to(BF16) if mode in ("residual", "rows") and not swiglu else None
    rows = torch.randperm(Mtot, generator=g)[:M] if mode == "rows" else None
    return x, W, swiglu, bias, R, rows, Nout


def _cases():
    """Every mode on every shape, except where the model has no such launch and the CPU side is dear: the gate+up shape carries only the SwiGLU
    epilogue (alone and through a row list), the down projection (K = 18 944: seconds of CPU per restatement) no bias and no SwiGLU."""
    out = []
    for M, N, K in SHAPES:
        for mode in MODES:
            if (K == 18944 and mode in ("bias", "swiglu")) or (N == 37888 and mode in ("plain", "bias", "residual")):
                continue
            out.append(pytest.param(M, N, K, mode, id=f"{mode}-{M}x{N}x{K}"))
    return out


@pytest.mark.parametrize("M,N,K,mode", _cases())
def test_gemm_w4_matches_restatement(M, N, K, mode):
    o = ops()
    x, W, swiglu, bias, R, rows, Nout = _case(M, N, K, mode, seed=M + N + K)
    q, s = o.quantize_rows_mxfp4(W.to(DEV))
    qr, sr = MX.quantize_mxfp4(W)
    assert torch.equal(q.cpu(), qr) and torch.equal(s.cpu(), MX.permute_scales(sr))
    aq, sa = o.quantize_rows_fp8(x.to(DEV))
    SENT = 7.0
    C = torch.full((x.shape[0], Nout), SENT, dtype=BF16, device=DEV)
    if R is not None:
        C.copy_(R)                                                   # the residual is read in place, through the same row list
    o.gemm_w4(aq, sa, q, s, C, bias=None if bias is None else bias.to(DEV), rows=None if rows is None else rows.to(DEV, torch.int32),
              residual=C if R is not None else None, epilogue=o.EPI_SWIGLU16 if swiglu else o.EPI_NONE)
    torch.cuda.synchronize()
    got = C.cpu()
    sel = torch.arange(x.shape[0]) if rows is None else rows
    if rows is not None:                                             # rows the list does not name come back untouched
        keep = torch.ones(x.shape[0], dtype=torch.bool)
        keep[rows] = False
        assert torch.equal(got[keep], (R if R is not None else torch.full_like(got, SENT))[keep]), "a row outside the row list was written"
    if N > 8192:                                                     # sampled whole 32-row weight blocks (see the module docstring)
        blocks = torch.tensor([0, 1, 7, 8, 15, 16, 500, 777, N // 32 - 2, N // 32 - 1])
        wrows = (blocks[:, None] * 32 + torch.arange(32)[None]).reshape(-1)
        ocols = (blocks[:, None] * 16 + torch.arange(16)[None]).reshape(-1)
        ref = MX.gemv_w4(x[sel], qr[wrows], sr[wrows], swiglu=True)
        got = got[:, ocols]
    else:
        ref = MX.gemv_w4(x[sel], qr, sr, bias=bias, residual=None if R is None else R[sel], swiglu=swiglu)
    close(got[sel], ref, ulps=2, what=f"gemm_w4 {mode} M={M} N={N} K={K}")


def test_gemm_w4_two_row_groups_of_a_stream_batched_forward():
    """M >= 16 392 through two row groups with different weights: what a stream-batched denoise forward issues per projection (text rows on the und
    expert, latent rows on the gen expert), both calls writing one C."""
    o = ops()
    Mtot, K, N = 16400, 3584, 256
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(Mtot, K, generator=g) * 1.5).to(BF16)
    W = [(torch.randn(N, K, generator=g) * K ** -0.5).to(BF16) for _ in range(2)]
    bias = [(torch.randn(N, generator=g) * 0.1).to(BF16) for _ in range(2)]
    perm = torch.randperm(Mtot, generator=g)
    groups = [perm[:8].sort().values, perm[8:].sort().values]                  # 8 marker rows, 16 392 latent rows
    aq, sa = o.quantize_rows_fp8(x.to(DEV))
    C = torch.full((Mtot, N), float("nan"), dtype=BF16, device=DEV)
    ref = torch.empty(Mtot, N, dtype=BF16)
    for w, b, r in zip(W, bias, groups):
        q, s = o.quantize_rows_mxfp4(w.to(DEV))
        o.gemm_w4(aq, sa, q, s, C, bias=b.to(DEV), rows=r.to(DEV, torch.int32))
        ref[r] = MX.gemv_w4(x[r], *MX.quantize_mxfp4(w), bias=b)
    torch.cuda.synchronize()
    close(C.cpu(), ref, ulps=2, what="gemm_w4 two row groups")


@pytest.mark.parametrize("M,N,K", [(100, 160, 640), (129, 288, 128), (16, 32, 2048)])
def test_gemm_w4_exact_integers(M, N, K):
    """Operand layout: e4m3-exact integer activations (|a| <= 3) with sa = 1 against hand-built random codes and power-of-two block scales
    (2^-1 .. 2^2) of an ASYMMETRIC W.  Every product is a multiple of 2^-2 and every partial sum stays below 2^18, so the fp32 accumulation is
    exact in any order and the bf16 output is the one correctly rounded value: a swapped nibble, a mis-ordered scale byte or a transposed C
    write cannot pass."""
    o = ops()
    g = torch.Generator().manual_seed(K)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    codes = torch.randint(0, 16, (N, K), generator=g).to(torch.uint8)
    packed = (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()
    sb = torch.tensor([126, 127, 128, 129], dtype=torch.uint8)[torch.randint(0, 4, (N, K // 32), generator=g)]
    ref = a.double() @ MX.dequant_mxfp4(packed, sb).double().t()
    assert ref.abs().max() < 2 ** 18 and torch.equal(ref.float().double(), ref)
    aq = a.to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(aq.view(torch.float8_e4m3fn).float(), a)
    C = torch.full((M, N), float("nan"), dtype=BF16, device=DEV)
    o.gemm_w4(aq.to(DEV), torch.ones(M, dtype=torch.float32, device=DEV), packed.to(DEV), MX.permute_scales(sb).to(DEV), C)
    torch.cuda.synchronize()
    bad = (C.cpu() != ref.float().to(BF16))
    assert not bad.any(), f"{bad.sum().item()} of {bad.numel()} outputs differ; first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("M", [1, 2, 4])
@pytest.mark.parametrize("mode", ["plain", "swiglu", "residual"])
def test_gemm_w4_agrees_with_gemv_w4_on_few_rows(M, mode):
    """The decode kernel and the GEMM read one stored copy of the codes: same product on M <= 4 rows."""
    o = ops()
    N, K = 1024, 3584
    g = torch.Generator().manual_seed(M)
    x = (torch.randn(M, K, generator=g) * 1.5).to(BF16).to(DEV)
    q, s = o.quantize_rows_mxfp4((torch.randn(N, K, generator=g) * K ** -0.5).to(BF16).to(DEV))
    swiglu = mode == "swiglu"
    Nout = N // 2 if swiglu else N
    R = torch.randn(M, Nout, generator=g).to(BF16).to(DEV) if mode == "residual" else None
    epi = o.EPI_SWIGLU16 if swiglu else o.EPI_NONE
    Cv = torch.empty((M, Nout), dtype=BF16, device=DEV)
    Cm = torch.empty((M, Nout), dtype=BF16, device=DEV)
    o.gemv_w4(x, q, s, Cv, residual=R, epilogue=epi)
    aq, sa = o.quantize_rows_fp8(x)
    o.gemm_w4(aq, sa, q, s, Cm, residual=R, epilogue=epi)
    torch.cuda.synchronize()
    close(Cm, Cv, ulps=2, what=f"gemm_w4 vs gemv_w4 {mode} M={M}")


def test_gemm_w4_nan_row_stays_in_its_row():
    o = ops()
    M, N, K = 40, 256, 512
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, K, generator=g).to(BF16)
    x[5, 17] = float("nan")
    q, s = o.quantize_rows_mxfp4((torch.randn(N, K, generator=g) * K ** -0.5).to(BF16).to(DEV))
    aq, sa = o.quantize_rows_fp8(x.to(DEV))
    C = torch.zeros((M, N), dtype=BF16, device=DEV)
    o.gemm_w4(aq, sa, q, s, C)
    torch.cuda.synchronize()
    c = C.cpu().float()
    assert torch.isnan(c[5]).all(), "the NaN activation row must give a NaN output row"
    others = torch.cat([c[:5], c[6:]])
    assert torch.isfinite(others).all() and others.abs().max() > 0, "its neighbours must stay finite"


def test_gemm_w4_refuses_bad_shapes():
    from bagel_amd._lib import BagelHipError
    o = ops()
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=DEV)  # noqa: E731
    sa = torch.ones(8, dtype=torch.float32, device=DEV)
    with pytest.raises(BagelHipError):                               # K % 128
        o.gemm_w4(u8(8, 192), sa, u8(16, 96), u8(16, 16), torch.empty((8, 16), dtype=BF16, device=DEV))
    with pytest.raises(BagelHipError):                               # N % 8
        o.gemm_w4(u8(8, 128), sa, u8(12, 64), u8(12, 16), torch.empty((8, 12), dtype=BF16, device=DEV))
    with pytest.raises(BagelHipError):                               # SwiGLU: N % 32
        o.gemm_w4(u8(8, 128), sa, u8(16, 64), u8(16, 16), torch.empty((8, 8), dtype=BF16, device=DEV), epilogue=o.EPI_SWIGLU16)
