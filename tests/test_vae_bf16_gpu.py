"""Per-kernel GPU tests of the bf16 VAE path (bagel_conv_gemm_bf16, bagel_groupnorm_bf16, bagel_softmax_rows_bf16,
bagel_vae_reparam_bf16): each kernel against a float64 reference of the same operation under a PER-ELEMENT bound derived from the
number formats (tests/util_vae_ref.py states and derives them; tests/test_vae_bf16_ref_cpu.py validates them without a GPU).
A single wrong border pixel, pad column or rounding fails.  Every test prints its worst error / bound ratio.
"""
import pytest
import torch

from tests import util_vae_ref as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F32 = torch.float32
DEV = "cuda"
EXTRA_ROWS = 128


def ops():
    from bagel_amd import ops as o
    return o


def _ceil_to(x, m):
    return (x + m - 1) // m * m


def sentinel(rows, cols, f32=False):
    if f32:
        return torch.full((rows, cols), R.SENTINEL_F32, dtype=torch.int32, device=DEV).view(F32)
    return torch.full((rows, cols), R.SENTINEL_BF16, dtype=torch.int16, device=DEV).view(BF16)


def untouched(t):
    bits = t.view(torch.int32 if t.dtype == F32 else torch.int16)
    return bool((bits == (R.SENTINEL_F32 if t.dtype == F32 else R.SENTINEL_BF16)).all())


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def run_conv(x, w, bias, res, mode, cout, f32=False):
    """One 3x3 launch as VaeEngineBf16.conv makes it (ld_out = Cout rounded up to 8) into a sentinel-filled buffer with EXTRA_ROWS
    spare rows; returns the [B, Ho, Wo, Cout] result after checking that pad columns and spare rows kept the sentinel."""
    B, H, W, cin = x.shape
    Ho, Wo = R.conv_out_hw(H, W, mode)
    M = B * Ho * Wo
    ld = _ceil_to(cout, 8)
    buf = sentinel(M + EXTRA_ROWS, ld, f32)
    ops().conv_gemm_bf16(dev(x), cin, dev(w), w.shape[1], dev(bias), dev(res), buf, ld, B, H, W, cin, Ho, Wo, cout, mode)
    torch.cuda.synchronize()
    assert untouched(buf[M:]), "rows behind the last pixel were written"
    assert untouched(buf[:M, cout:]), "pad columns Cout..ld_out-1 were written"
    return buf[:M, :cout].cpu().view(B, Ho, Wo, cout)


# ---- 1. exact tap addressing ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("cin", [24, 64])
def test_conv_taps_exact(mode, cin):
    """Integer-coded input through one-hot weights: the output IS the shifted input, bit for bit, and exactly 0 where a tap leaves
    the image.  B = 2, 9 x 13: two pixel tiles with a tail (mode 1), odd sizes (mode 2); Cin = 24: per-chunk taps, K = 216 with taps
    straddling k-tiles and a K tail; Cin = 64: one tap per k-tile, Cout = 576 -> 10 blocks (mode 1: the XCD remap at remainder 2)."""
    x = R.tap_code_input(2, 9, 13, cin)
    got = run_conv(x, R.onehot_weights(cin), None, None, mode, 9 * cin)
    exp = R.tap_expected(x, mode)
    wrong = (got.view(torch.int16) != exp.view(torch.int16)) & ~((got == 0) & (exp == 0))      # +0 only comes out of the kernel; -0 never
    print(f"taps mode {mode} cin {cin}: {int(wrong.sum())} of {wrong.numel()} elements differ")
    if wrong.any():
        b, y, xx, c = [int(v) for v in wrong.nonzero()[0]]
        raise AssertionError(f"mode {mode}: {int(wrong.sum())} wrong elements, first at (b, y, x) = ({b}, {y}, {xx}), tap {c // cin}, ci {c % cin}: "
                             f"got {got[b, y, xx, c].item()}, expected {exp[b, y, xx, c].item()}")


# ---- 2. random conv under the derived bound -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("cin,cout,H,W", R.CONV_CASES)
def test_conv_random(mode, cin, cout, H, W):
    worst = 0.0
    for bias, residual in R.conv_variants(cout):
        x, w4, b, r = R.conv_inputs(R.conv_seed(mode, cin, cout), 2, H, W, cin, cout, mode, bias, residual)
        got = run_conv(x, R.pack_w(w4), b, None if r is None else r.view(-1, cout), mode, cout)
        t, A = R.conv_ref(x, w4, b, mode)
        ratio = R.conv_check(got, t, A, 9 * cin, r)
        print(f"conv mode {mode} cin {cin} cout {cout} {H}x{W} bias {bias} residual {residual}: error / bound = {ratio:.3f}")
        worst = max(worst, ratio)
    assert worst <= 1.0, f"worst error / bound = {worst}"


# ---- 3. mode 0: plain GEMM ------------------------------------------------------------------------------------------------
def run_gemm(a, w, bias, res, f32, pad_in=0, pad_out=0, spare_rows=EXTRA_ROWS):
    """a [M, K] as a view of [M, K + pad_in] rows (the pad holds 3e4: a read across a row end shows), out a view of [M, N + pad_out]."""
    M, K = a.shape
    N = w.shape[0]
    abuf = torch.full((M, K + pad_in), 3e4, dtype=BF16, device=DEV)
    abuf[:, :K] = a.to(DEV)
    out = sentinel(M + spare_rows, N + pad_out, f32)
    rbuf = None
    if res is not None:
        rbuf = torch.zeros((M, N + pad_out), dtype=BF16, device=DEV)
        rbuf[:, :N] = res.to(DEV)
    ops().conv_gemm_bf16(abuf[:, :K], K + pad_in, dev(w), K, dev(bias), rbuf, out, N + pad_out, 1, 1, M, K, 1, M, N, 0)
    torch.cuda.synchronize()
    assert untouched(out[M:]) and untouched(out[:M, N:])
    return out[:M, :N].cpu()


@pytest.mark.parametrize("M,N,K,f32,pad_in,pad_out", R.GEMM_CASES)
def test_gemm_mode0(M, N, K, f32, pad_in, pad_out):
    a, w, _, _ = R.gemm_inputs(M + N + K, M, N, K)
    got = run_gemm(a, w, None, None, f32, pad_in, pad_out)
    assert got.dtype == (F32 if f32 else BF16)
    t, A = R.gemm_ref(a, w)
    ratio = R.conv_check(got, t, A, K, out_f32=f32)
    print(f"gemm {M}x{N}x{K} f32 {f32} ld_in {K + pad_in} ld_out {N + pad_out}: error / bound = {ratio:.3f}")
    assert ratio <= 1.0


def test_gemm_bias_residual_as_proj_out():
    a, w, b, r = R.gemm_inputs(7, 234, 64, 64, bias=True, residual=True)
    got = run_gemm(a, w, b, r, False)
    t, A = R.gemm_ref(a, w, b)
    ratio = R.conv_check(got, t, A, 64, r)
    print(f"gemm 234x64x64 bias + residual: error / bound = {ratio:.3f}")
    assert ratio <= 1.0


def test_gemm_attention_call_pattern():
    """The three launches of VaeEngineBf16.attn at N = 35 (N8 = 40), C = 64: scores into an [R, N8] fp32 buffer, bf16 probabilities
    into a zeroed [R, N8] buffer, probabilities x vt[C, N8]; each stage against the float64 reference of ITS OWN inputs."""
    N, N8, C, Rr = 35, 40, 64, 48
    g = R.gen(35)
    q, k, v = R.randn_bf16(g, N, C), R.randn_bf16(g, N, C), R.randn_bf16(g, N, C)
    sbuf, pbuf = sentinel(Rr, N8, True), torch.zeros((Rr, N8), dtype=BF16, device=DEV)
    qd, kd = dev(q), dev(k)
    vt = torch.zeros((C, N8), dtype=BF16, device=DEV)
    vt[:, :N] = v.to(DEV).t()
    o = sentinel(N + EXTRA_ROWS, C)
    s, pr = sbuf[:N], pbuf[:N]
    ops().conv_gemm_bf16(qd, C, kd, C, None, None, s, N8, 1, 1, N, C, 1, N, N, 0)
    ops().softmax_rows_bf16(s, pr, N, N, float(C) ** -0.5)
    ops().conv_gemm_bf16(pr, N8, vt, N8, None, None, o, C, 1, 1, N, N8, 1, N, C, 0)
    torch.cuda.synchronize()
    assert untouched(sbuf[N:]) and untouched(sbuf[:N, N:]) and untouched(o[N:])
    assert bool((pbuf[:, N:] == 0).all()) and bool((pbuf[N:] == 0).all())
    sc, p, og = sbuf[:N, :N].cpu(), pbuf[:N, :N].cpu(), o[:N].cpu()
    t, A = R.gemm_ref(q, k)
    r1 = R.conv_check(sc, t, A, C, out_f32=True)
    r2 = R.worst_ratio(p, *R.softmax_ref(sc, float(C) ** -0.5))
    t, A = R.gemm_ref(p, v.t().contiguous())
    r3 = R.conv_check(og, t, A, N8)
    print(f"attention pattern: scores {r1:.3f}, probabilities {r2:.3f}, P V {r3:.3f} (error / bound)")
    assert max(r1, r2, r3) <= 1.0


# ---- 4. argument contract ---------------------------------------------------------------------------------------------------
def test_conv_argument_contract():
    from bagel_amd._lib import BagelHipError
    o = ops()
    x, w = torch.zeros((2 * 4 * 4, 16), dtype=BF16, device=DEV), torch.zeros((8, 9 * 16), dtype=BF16, device=DEV)
    bias, res = torch.zeros(8, dtype=BF16, device=DEV), torch.zeros((32, 8), dtype=BF16, device=DEV)
    out, out32 = sentinel(32, 8), sentinel(32, 8, True)
    with pytest.raises(BagelHipError):                      # Cin % 8 != 0
        o.conv_gemm_bf16(x, 12, w, 9 * 16, None, None, out, 8, 2, 4, 4, 12, 4, 4, 8, 1)
    with pytest.raises(BagelHipError):                      # ld_out % 4 != 0
        o.conv_gemm_bf16(x, 16, w, 9 * 16, None, None, out, 6, 2, 4, 4, 16, 4, 4, 6, 1)
    with pytest.raises(BagelHipError):                      # fp32 output takes no bias
        o.conv_gemm_bf16(x, 16, w, 9 * 16, bias, None, out32, 8, 2, 4, 4, 16, 4, 4, 8, 1)
    with pytest.raises(BagelHipError):                      # ... and no residual
        o.conv_gemm_bf16(x, 16, w, 9 * 16, None, res, out32, 8, 2, 4, 4, 16, 4, 4, 8, 1)
    o.conv_gemm_bf16(x, 16, w, 9 * 16, bias, None, out, 8, 0, 4, 4, 16, 4, 4, 8, 1)       # M = 0
    o.conv_gemm_bf16(x, 16, w, 9 * 16, bias, None, out, 8, 2, 4, 4, 16, 4, 4, 0, 1)       # Cout = 0
    torch.cuda.synchronize()
    assert untouched(out) and untouched(out32)


# ---- 5. GroupNorm ---------------------------------------------------------------------------------------------------------------
def run_gn(x, gamma, beta, swish):
    """-> (result [B, HW, C] on the CPU, the kernel's (mean, rstd) [B, 32, 2] read back from its workspace (include/bagel_hip.h layout))."""
    B, HW, C = x.shape
    ws = torch.zeros(ops().groupnorm_bf16_workspace_floats(B, C, 32), dtype=F32, device=DEV)
    y = sentinel(1, B * HW * C + 1024)
    ops().groupnorm_bf16(dev(x), y, ws, dev(gamma), dev(beta), B, HW, C, 32, 1e-6, swish)
    torch.cuda.synchronize()
    assert untouched(y[:, B * HW * C:])
    return y[0, :B * HW * C].cpu().view(B, HW, C), ws[B * 32 * 2048:B * 32 * 2050].cpu().view(B, 32, 2)


def gn_check(x, gamma, beta, swish, what):
    got, stats = run_gn(x, gamma, beta, swish)
    ref, bound = R.gn_ref(x, gamma, beta, swish)
    ratio = R.worst_ratio(got, ref, bound)
    mean, rstd = R.gn_stats_ref(x)
    e_rstd = ((stats[..., 1].double() - rstd).abs() / rstd).max().item()
    e_mean = ((stats[..., 0].double() - mean).abs() * rstd).max().item()
    print(f"groupnorm {what} swish {swish}: error / bound = {ratio:.3f}, rstd relative error {e_rstd:.3g}, mean error in sigmas {e_mean:.3g}")
    return ratio


@pytest.mark.parametrize("swish", [False, True])
@pytest.mark.parametrize("C,HW", R.GN_SHAPES)
def test_groupnorm(C, HW, swish):
    """C = 64, 128, 512: the coalesced statistics kernel; 96, 160: the per-group one.  HW = 16: one slice of fewer than 64 pixels;
    240: 3 slices; 130: 2 slices of 65; 6401: 100 slices of 65 pixels, slice 98 partial and slice 99 empty."""
    x, gamma, beta = R.gn_inputs(C + HW, 2, HW, C)
    assert gn_check(x, gamma, beta, swish, f"C {C} HW {HW}") <= 1.0


@pytest.mark.parametrize("C,kind", R.GN_OUTLIER_CASES)
def test_groupnorm_outlier(C, kind):
    """N(0, 0.05^2) with one element of 200 per group.  At pixel 0 it is the group's first element: statistics shifted by that element
    (s2 / n - md^2 around a pivot 4000 sigmas away) lose about 4e-3 of rstd, a whole bf16 ulp of the result; at pixel 1234 the same data
    is harmless for such a scheme, which shows that the bound is not what fails."""
    x, gamma, beta = R.gn_inputs(C, 2, R.GN_OUTLIER_HW, C, kind)
    assert gn_check(x, gamma, beta, False, f"C {C} {kind}") <= 1.0


# ---- 6. softmax -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", R.SOFTMAX_COLS)
def test_softmax(cols):
    o = ops()
    for kind in ("normal", "wide", "equal"):
        x, scale = R.softmax_inputs(cols, 3, cols, kind)
        xb = torch.full((3, cols + 3), 1e30, dtype=F32, device=DEV)         # x.stride(0) > cols; a read past the row end would win the max
        xb[:, :cols] = x.to(DEV)
        yb = sentinel(4, cols + 5)
        o.softmax_rows_bf16(xb[:, :cols], yb[:3, :cols], 3, cols, scale)
        torch.cuda.synchronize()
        assert untouched(yb[3:]) and untouched(yb[:3, cols:])
        got = yb[:3, :cols].cpu()
        ratio = R.worst_ratio(got, *R.softmax_ref(x, scale))
        print(f"softmax cols {cols} {kind}: error / bound = {ratio:.3f}")
        assert ratio <= 1.0
        if kind == "equal":
            assert torch.equal(got, torch.full((3, cols), 1.0 / cols, dtype=F32).to(BF16))
    o.softmax_rows_bf16(xb[:, :cols], yb[3:, :cols], 0, cols, 0.25)            # rows = 0
    torch.cuda.synchronize()
    assert untouched(yb[3:])


# ---- 7. reparam -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("zc,ld", R.REPARAM_CASES)
def test_reparam_bit_equal(zc, ld, with_noise):
    mom, noise = R.reparam_inputs(R.REPARAM_SEED, R.N_PIX, zc, ld)
    nz = noise if with_noise else None
    md = dev(mom)[:, :2 * zc]                               # zc = 4: a view of 16-wide rows
    assert md.stride(0) == ld
    z = sentinel(1, R.N_PIX * zc + 64)
    ops().vae_reparam_bf16(md, dev(nz), z, R.N_PIX, zc, R.SCALE_FACTOR, R.SHIFT_FACTOR)
    torch.cuda.synchronize()
    assert untouched(z[:, R.N_PIX * zc:])
    got = z[0, :R.N_PIX * zc].cpu().view(R.N_PIX, zc)
    ref = R.reparam_ref(mom, nz, zc)
    diff = int((got.view(torch.int16) != ref.view(torch.int16)).sum())
    print(f"reparam zc {zc} ld {ld} noise {with_noise}: {diff} of {ref.numel()} elements differ from eager bf16")
    assert diff == 0


@pytest.mark.parametrize("zc,ld", R.REPARAM_CASES)
def test_reparam_reference_is_eager_bf16_on_the_device(zc, ld):
    """The literal eager expression on the device gives the bits of the CPU reference (util_vae_ref.reparam_ref explains the one op
    that the CPU backend rounds differently)."""
    mom, noise = R.reparam_inputs(R.REPARAM_SEED, R.N_PIX, zc, ld)
    assert torch.equal(R.reparam_eager(dev(mom), dev(noise), zc).cpu(), R.reparam_ref(mom, noise, zc))


# ---- 8. the attention block through the engine ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(5, 7), (8, 8)])
def test_attn_block(H, W):
    from bagel_amd.modeling.autoencoder import AutoEncoder, AutoEncoderParams
    from bagel_amd.modeling.vae_engine import VaeEngineBf16
    from oracle.configs import TINY
    from oracle.weights import load_synth
    ae = AutoEncoder(AutoEncoderParams(**TINY["vae"]))
    load_synth(ae, 0)
    m = ae.encoder.mid.attn_1
    C = m.q.weight.shape[0]
    x = R.randn_bf16(R.gen(H * W), 2, H, W, C)
    ref = R.attn_block_ref(x, m)
    ae = ae.to(DEV)
    eng = VaeEngineBf16(ae)
    a = eng.attn(dev(x), ae.encoder.mid.attn_1).cpu()
    eng.ATTN_ROWS = 16                                      # 35 = 16 + 16 + 3, 64 = 4 x 16: the row-block loop, with a remainder block
    b = eng.attn(dev(x), ae.encoder.mid.attn_1).cpu()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "the result depends on the score block size"
    d, l2 = R.chained_check(a, ref)
    print(f"attention block {H}x{W}: max|d| / allowed = {d:.3f}, rel-L2 / allowed = {l2:.3f}")
    assert d <= 1.0 and l2 <= 1.0
