"""The references and bounds of tests/test_vae_bf16_gpu.py, validated without a GPU (tests/util_vae_ref.py).

A plain fp32 torch stand-in for each bf16 VAE kernel (another summation order, the same rounding points) must pass every bound the GPU
file uses, on the same seeded inputs; stand-ins that are wrong in the ways the bounds are meant to catch -- one border tap dropped at
one pixel, the two roundings of the residual add merged into one, a GroupNorm slice left out of the statistics -- must fail them.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import util_vae_ref as R

BF16 = torch.bfloat16


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("cin,cout,H,W", R.CONV_CASES)
def test_conv_standin_passes_and_wrong_standins_fail(mode, cin, cout, H, W):
    K = 9 * cin
    for bias, residual in R.conv_variants(cout):
        x, w4, b, r = R.conv_inputs(R.conv_seed(mode, cin, cout), 2, H, W, cin, cout, mode, bias, residual)
        t, A = R.conv_ref(x, w4, b, mode)
        ratio = R.conv_check(R.conv_standin(x, w4, b, mode, r), t, A, K, r)
        print(f"mode {mode} cin {cin} cout {cout} bias {bias} residual {residual}: stand-in error / bound = {ratio:.3f}")
        assert ratio <= 1.0
        dropped = R.conv_check(R.conv_standin(x, w4, b, mode, r, drop_border_tap=True), t, A, K, r)
        assert dropped > 1.0, "a tap dropped at ONE border pixel must fail the per-element bound"
        if residual:
            merged = R.conv_check(R.conv_standin(x, w4, b, mode, r, merge_roundings=True), t, A, K, r)
            assert merged > 1.0, "bf16(t + r) instead of bf16(bf16(t) + r) must fail"


def test_conv_bound_is_tight():
    """The accumulation term is a small fraction of the rounding term: at the median the whole bound stays below 1e-2 |ref|."""
    for cin in (24, 64, 160):
        x, w4, b, _ = R.conv_inputs(5, 2, 9, 13, cin, 16, 1)
        t, A = R.conv_ref(x, w4, b, 1)
        _, bound = R.conv_bound(t, A, 9 * cin)
        assert (bound / t.abs()).median().item() < 1e-2


@pytest.mark.parametrize("M,N,K,f32,pad_in,pad_out", R.GEMM_CASES)
def test_gemm_standin_passes(M, N, K, f32, pad_in, pad_out):
    a, w, _, _ = R.gemm_inputs(M + N + K, M, N, K)
    t, A = R.gemm_ref(a, w)
    assert R.conv_check(R.gemm_standin(a, w, out_f32=f32), t, A, K, out_f32=f32) <= 1.0
    a, w, b, r = R.gemm_inputs(7, 234, 64, 64, bias=True, residual=True)
    t, A = R.gemm_ref(a, w, b)
    assert R.conv_check(R.gemm_standin(a, w, b, r), t, A, 64, r) <= 1.0


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("cin", [24, 64])
def test_tap_expected_matches_conv2d(mode, cin):
    """The index-arithmetic expectation of the one-hot conv equals F.conv2d on the same operands (all values are small integers: exact)."""
    x = R.tap_code_input(2, 9, 13, cin)
    assert x.abs().max().item() <= 125 and x.float().frac().abs().max().item() == 0
    w4 = R.onehot_weights(cin).view(9 * cin, 3, 3, cin).permute(0, 3, 1, 2)
    assert torch.equal(R.pack_w(w4), R.onehot_weights(cin))
    t, _ = R.conv_ref(x, w4, None, mode, dtype=torch.float32)
    exp = R.tap_expected(x, mode)
    assert exp.shape == t.shape and torch.equal(exp.float(), t)
    Ho, Wo = R.conv_out_hw(9, 13, mode)
    if mode != 2:
        assert exp[:, 0, :, :3 * cin].abs().max().item() == 0       # the dy = 0 taps of the top row leave the image
    else:
        assert exp[:, :, Wo - 1, 2 * cin:3 * cin].abs().max().item() != 0 and Ho == 4 and Wo == 6      # 2 * 5 + 2 = 12 < 13: still inside


@pytest.mark.parametrize("swish", [False, True])
@pytest.mark.parametrize("C,HW", [(64, 16), (128, 240), (96, 130), (512, 130)])
def test_groupnorm_standin_passes_and_dropped_slice_fails(C, HW, swish):
    x, gamma, beta = R.gn_inputs(C + HW, 2, HW, C)
    ref, bound = R.gn_ref(x, gamma, beta, swish)
    assert R.worst_ratio(R.gn_standin(x, gamma, beta, swish), ref, bound) <= 1.0
    if HW == 130:
        # statistics over the second slice of 65 pixels only, applied to everything
        mean, rstd = R.gn_stats_ref(x[:, 65:])
        cpg = C // 32
        a = rstd.repeat_interleave(cpg, 1) * gamma.double()
        y = a.view(2, 1, C) * x.double() + (beta.double() - mean.repeat_interleave(cpg, 1) * a).view(2, 1, C)
        if swish:
            y = y * torch.sigmoid(y)
        assert R.worst_ratio(y.to(BF16), ref, bound) > 1.0


@pytest.mark.parametrize("C,kind", R.GN_OUTLIER_CASES)
def test_groupnorm_outlier_standin_passes_and_rstd_off_by_a_bf16_ulp_fails(C, kind):
    x, gamma, beta = R.gn_inputs(C, 2, R.GN_OUTLIER_HW, C, kind)
    pix = 0 if kind == "pivot0" else 1234
    assert (x[:, pix, ::C // 32] == 200).all() and (x.abs() == 200).sum().item() == 2 * 32
    ref, bound = R.gn_ref(x, gamma, beta, False)
    assert R.worst_ratio(R.gn_standin(x, gamma, beta, False), ref, bound) <= 1.0
    # rstd wrong by 2^-8 relative (the size of the loss a first-element pivot suffers here)
    mean, rstd = R.gn_stats_ref(x)
    cpg = C // 32
    a = (rstd * (1 + 2.0 ** -8)).repeat_interleave(cpg, 1) * gamma.double()
    y = a.view(2, 1, C) * x.double() + (beta.double() - mean.repeat_interleave(cpg, 1) * a).view(2, 1, C)
    assert R.worst_ratio(y.to(BF16), ref, bound) > 1.0


@pytest.mark.parametrize("cols", R.SOFTMAX_COLS)
def test_softmax_standin_passes(cols):
    for kind in ("normal", "wide", "equal"):
        x, scale = R.softmax_inputs(cols, 3, cols, kind)
        ref, bound = R.softmax_ref(x, scale)
        got = R.softmax_standin(x, scale)
        assert R.worst_ratio(got, ref, bound) <= 1.0, kind
        if kind == "wide":
            assert cols == 1 or (x.max() - x.min()).item() * scale > 30        # without the max subtraction exp would overflow or vanish
            assert (x.abs().max().item() * scale <= 100)
        if kind == "equal":
            assert torch.equal(got, torch.full((3, cols), 1.0 / cols, dtype=torch.float32).to(BF16))


@pytest.mark.parametrize("zc,ld", R.REPARAM_CASES)
def test_reparam_reference_is_the_kernel_formula_and_no_exp_near_a_midpoint(zc, ld):
    mom, noise = R.reparam_inputs(R.REPARAM_SEED, R.N_PIX, zc, ld)
    lv = mom[:, zc:2 * zc].float()
    assert lv.min().item() >= -8 and lv.max().item() <= 4
    for nz in (noise, None):
        ref = R.reparam_ref(mom, nz, zc)
        assert ref.dtype == BF16 and ref.shape == (R.N_PIX, zc)
        assert torch.equal(ref, R.reparam_emulated(mom, nz, zc))
    # the one place where the reference is not the literal CPU expression: only the scalar of the subtraction is treated differently
    z = mom[:, :zc] + torch.exp(0.5 * mom[:, zc:2 * zc]) * noise
    assert torch.equal(R.reparam_eager(mom, noise, zc), R.SCALE_FACTOR * (z.float() - torch.tensor(R.SHIFT_FACTOR).to(BF16).float()).to(BF16))
    # a device expf may differ from the host's only in the last fp32 bits; no exp here is that close to a bf16 rounding midpoint,
    # so the GPU test excuses nothing
    assert R.reparam_exp_midpoint_margin(mom, zc) > 2.0 ** -20


def test_reparam_midpoint_margin_measures_the_distance():
    mom = torch.zeros(1, 2, dtype=BF16)                  # exp(0) = 1 = 256 * 2^-8: the midpoint above it is 1 + 2^-8
    assert abs(R.reparam_exp_midpoint_margin(mom, 1) - 2.0 ** -8) < 1e-12
    # exp(0.5 * 1) = 1.64872 = 2 * 0.82436, and 0.82436 = 422.07 * 2^-9: the nearest odd multiple of 2^-9 (a midpoint of the 2^-8 grid) is 423
    e = torch.exp(torch.tensor(0.5, dtype=torch.float64)).item()
    assert abs(R.reparam_exp_midpoint_margin(torch.tensor([[0.0, 1.0]], dtype=BF16), 1) - (423 - e * 256) / (e * 256)) < 1e-9


def _attn_module():
    from bagel_amd.modeling.autoencoder import AutoEncoder, AutoEncoderParams
    from oracle.configs import TINY
    from oracle.weights import load_synth
    ae = AutoEncoder(AutoEncoderParams(**TINY["vae"]))
    load_synth(ae, 0)
    return ae.encoder.mid.attn_1


@pytest.mark.parametrize("H,W", [(5, 7), (8, 8)])
def test_attn_reference_against_fp32_torch_with_the_same_cast_points(H, W):
    m = _attn_module()
    C = m.q.weight.shape[0]
    x = R.randn_bf16(R.gen(H * W), 2, H, W, C)
    ref = R.attn_block_ref(x, m)
    xs = x.view(2, H * W, C)
    h = F.group_norm(xs.float().permute(0, 2, 1), 32, m.norm.weight.data, m.norm.bias.data, 1e-6).permute(0, 2, 1).to(BF16)

    def lin(v, c):
        return (v.float() @ c.weight.data.reshape(C, C).to(BF16).float().t() + c.bias.data.to(BF16).float()).to(BF16)
    q, k, v = lin(h, m.q), lin(h, m.k), lin(h, m.v)
    p = torch.softmax(q.float() @ k.float().transpose(1, 2) * float(C) ** -0.5, -1).to(BF16)
    o = (p.float() @ v.float()).to(BF16)
    got = (lin(o, m.proj_out).float() + xs.float()).to(BF16).view(2, H, W, C)
    d, l2 = R.chained_check(got, ref)
    assert d <= 1.0 and l2 <= 1.0, (d, l2)
