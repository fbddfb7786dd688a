"""float64 references, input builders and per-element error bounds for the bf16 VAE kernels (bagel_amd/csrc/vae.hip).

Everything here runs on the CPU.  tests/test_vae_bf16_gpu.py compares the kernels against these references;
tests/test_vae_bf16_ref_cpu.py checks, without a GPU, that a plain fp32 torch implementation passes every bound and that
two deliberately wrong ones do not.

All inputs are drawn from a seeded torch.Generator and rounded to bf16 FIRST, so the reference and the kernel see the same
values and the bounds only have to cover what happens after that.

Bounds (all per element; `worst_ratio` returns max(error / bound), which a test prints and asserts <= 1):

  conv / GEMM   t = conv(x, w) + bias in float64, A = the same on absolute values, K = taps * Cin.
                bf16 out:      |got - t| <= 2^-8 |t| + 2 (K + 2) 2^-24 A
                  2^-8 |t| is the half-ulp of the one bf16 rounding; (K + 2) 2^-24 A is the worst case of K fp32
                  accumulations plus the bias add, doubled because the MFMA's internal order and rounding are not documented.
                bf16 out + residual r (the kernel computes bf16(bf16(t) + r)):
                               |got - (t + r)| <= 2^-8 (|t| + |t + r|) + 2 (K + 2) 2^-24 A
                  AND got inside [bf16(bf16(t - e) + r), bf16(bf16(t + e) + r)] with e the accumulation term: rounding is
                  monotone, so every legitimate result lies there; a single merged rounding bf16(t + r) does not.
                fp32 out:      |got - t| <= 2^-23 |t| + 2 (K + 2) 2^-24 A
  GroupNorm     a = rstd gamma, b = beta - mean a (float64, population variance):
                               |got - ref| <= 2^-8 |ref| + 2^-16 (|a x| + |b|)      (x 2 on the second term after swish)
                  2^-16 is 256 fp32 ulps of the operands: far above honest fp32 statistics (~1e-6), 1/256 of a bf16 ulp.
  softmax       |got - ref| <= (2^-8 + 2^-14) ref + 2^-126     (__expf argument error, |argument| <= 100)
  reparam       bit-equal to eager bf16 torch on the CPU
  chained       SURVEY.md 8c: max|d| <= 2 * 2^-7 * max|ref|, rel-L2 <= 4e-3
"""
import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
F64 = torch.float64
SENTINEL_BF16 = 0x7BCD       # a finite bf16 bit pattern (about 2.1e36) no result of these tests can take
SENTINEL_F32 = 0x7B3C5A69


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn_bf16(g, *shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=g) * scale + shift).to(BF16)


def rbf(x):
    """One rounding to bf16, back in float64."""
    return x.to(BF16).to(F64)


def worst_ratio(got, ref, bound):
    """max(|got - ref| / bound) over all elements; non-finite results count as infinitely wrong."""
    got, ref, bound = got.to(F64), ref.to(F64), bound.to(F64)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if not torch.isfinite(got).all():
        return float("inf")
    return ((got - ref).abs() / bound).max().item()


# ---------------------------------------------------------------------------------------------------------------------
# conv / GEMM
# ---------------------------------------------------------------------------------------------------------------------
def conv_out_hw(H, W, mode):
    return (H, W) if mode in (0, 1) else ((H // 2, W // 2) if mode == 2 else (2 * H, 2 * W))


def pack_w(w4):
    """[Cout, Cin, 3, 3] -> [Cout, 9 * Cin], tap-major (dy, dx, cin): the layout bagel_conv_gemm_bf16 reads."""
    return w4.permute(0, 2, 3, 1).reshape(w4.shape[0], -1).contiguous()


def _conv_nchw(x, w4, bias, mode):
    if mode == 1:
        return F.conv2d(x, w4, bias, padding=1)
    if mode == 2:
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w4, bias, stride=2)
    if mode == 3:
        return F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w4, bias, padding=1)
    raise ValueError(mode)


def conv_ref(x, w4, bias, mode, dtype=F64):
    """x [B, H, W, Cin] NHWC, w4 [Cout, Cin, 3, 3], bias [Cout] or None (bf16-valued) -> (t, A) NHWC in ``dtype``."""
    xn = x.to(dtype).permute(0, 3, 1, 2)
    b = None if bias is None else bias.to(dtype)
    t = _conv_nchw(xn, w4.to(dtype), b, mode)
    A = _conv_nchw(xn.abs(), w4.to(dtype).abs(), None if b is None else b.abs(), mode)
    return t.permute(0, 2, 3, 1).contiguous(), A.permute(0, 2, 3, 1).contiguous()


def gemm_ref(a, w, bias=None, dtype=F64):
    """a [M, K], w [N, K] -> (t, A) [M, N]."""
    t = a.to(dtype) @ w.to(dtype).t()
    A = a.to(dtype).abs() @ w.to(dtype).abs().t()
    if bias is not None:
        t, A = t + bias.to(dtype), A + bias.to(dtype).abs()
    return t, A


def acc_term(A, K):
    return 2.0 * (K + 2) * 2.0 ** -24 * A.to(F64)


def conv_bound(t, A, K, r=None, out_f32=False):
    """(reference, bound) of one conv / GEMM result, see the module docstring."""
    t = t.to(F64)
    e = acc_term(A, K)
    if out_f32:
        assert r is None
        return t, 2.0 ** -23 * t.abs() + e
    if r is None:
        return t, 2.0 ** -8 * t.abs() + e
    tr = t + r.to(F64)
    return tr, 2.0 ** -8 * (t.abs() + tr.abs()) + e


def residual_interval(t, A, K, r):
    """[lo, hi] (bf16) of bf16(bf16(u) + r) over every u within the accumulation term of t; the inner add in fp32 as the kernel does."""
    e = acc_term(A, K)
    rf = r.float()
    lo = ((t.to(F64) - e).to(BF16).float() + rf).to(BF16)
    hi = ((t.to(F64) + e).to(BF16).float() + rf).to(BF16)
    return lo, hi


def conv_check(got, t, A, K, r=None, out_f32=False):
    """Worst error / bound ratio of ``got``; with a residual a result outside the two-rounding interval counts as inf."""
    ref, bound = conv_bound(t, A, K, r, out_f32)
    ratio = worst_ratio(got, ref, bound)
    if r is not None:
        lo, hi = residual_interval(t, A, K, r)
        g = got.to(F64)
        if not bool(((g >= lo.to(F64)) & (g <= hi.to(F64))).all()):
            return float("inf")
    return ratio


def conv_standin(x, w4, bias, mode, r=None, out_f32=False, drop_border_tap=False, merge_roundings=False):
    """What the kernel computes, in plain fp32 torch (another summation order): fp32 accumulation, bf16(acc + bias), then
    bf16(. + r).  ``drop_border_tap`` loses the tap (dy, dx) = (1, 0) at the single output pixel (b, y, x) = (B - 1, 0, Wo - 1);
    ``merge_roundings`` rounds acc + bias + r once."""
    xn = x.float().permute(0, 3, 1, 2)
    acc = _conv_nchw(xn, w4.float(), None if bias is None else bias.float(), mode)
    if drop_border_tap:
        w1 = torch.zeros_like(w4.float())
        w1[:, :, 1, 0] = w4.float()[:, :, 1, 0]
        acc[-1, :, 0, -1] -= _conv_nchw(xn, w1, None, mode)[-1, :, 0, -1]
    acc = acc.permute(0, 2, 3, 1).contiguous()
    if out_f32:
        return acc
    if r is None:
        return acc.to(BF16)
    if merge_roundings:
        return (acc + r.float()).to(BF16)
    return (acc.to(BF16).float() + r.float()).to(BF16)


def gemm_standin(a, w, bias=None, r=None, out_f32=False):
    acc = a.float() @ w.float().t()
    if bias is not None:
        acc = acc + bias.float()
    if out_f32:
        return acc
    if r is None:
        return acc.to(BF16)
    return (acc.to(BF16).float() + r.float()).to(BF16)


def conv_inputs(seed, B, H, W, cin, cout, mode, bias=True, residual=False):
    """Seeded bf16 operands of one random conv case: x NHWC, w4, bias, residual (NHWC of the output shape)."""
    g = gen(seed)
    x = randn_bf16(g, B, H, W, cin)
    w4 = randn_bf16(g, cout, cin, 3, 3, scale=(9 * cin) ** -0.5)
    b = randn_bf16(g, cout, scale=0.1) if bias else None
    Ho, Wo = conv_out_hw(H, W, mode)
    r = randn_bf16(g, B, Ho, Wo, cout) if residual else None
    return x, w4, b, r


def gemm_inputs(seed, M, N, K, bias=False, residual=False):
    g = gen(seed)
    a = randn_bf16(g, M, K)
    w = randn_bf16(g, N, K, scale=K ** -0.5)
    b = randn_bf16(g, N, scale=0.1) if bias else None
    r = randn_bf16(g, M, N) if residual else None
    return a, w, b, r


# ---- exact tap addressing: integer-coded input, one-hot weights ---------------------------------------------------
def tap_code_input(B, H, W, cin):
    """x[b, y, x, c] = ((7 b + 5 y + 3 x + c) mod 251) - 125: integers of magnitude <= 125, exact in bf16."""
    b = torch.arange(B).view(B, 1, 1, 1)
    y = torch.arange(H).view(1, H, 1, 1)
    x = torch.arange(W).view(1, 1, W, 1)
    c = torch.arange(cin).view(1, 1, 1, cin)
    v = ((7 * b + 5 * y + 3 * x + c) % 251 - 125).to(BF16)
    assert torch.equal(v.double(), ((7 * b + 5 * y + 3 * x + c) % 251 - 125).double())
    return v


def onehot_weights(cin):
    """Packed [9 * cin, 9 * cin] identity: output channel tap * cin + ci has its single 1.0 at (tap, ci)."""
    return torch.eye(9 * cin, dtype=BF16)


def tap_expected(x, mode):
    """The exact output of the one-hot conv: out[b, y, x, tap * cin + ci] = the input at the tap's position, 0 outside the image.
    Written with explicit index arithmetic, independent of F.conv2d."""
    B, H, W, cin = x.shape
    Ho, Wo = conv_out_hw(H, W, mode)
    if mode == 3:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)        # nearest 2x
        H, W = 2 * H, 2 * W
    out = torch.zeros(B, Ho, Wo, 9 * cin, dtype=x.dtype)
    for dy in range(3):
        for dx in range(3):
            tap = dy * 3 + dx
            for yo in range(Ho):
                yy = 2 * yo + dy if mode == 2 else yo + dy - 1
                if not 0 <= yy < H:
                    continue
                for xo in range(Wo):
                    xx = 2 * xo + dx if mode == 2 else xo + dx - 1
                    if 0 <= xx < W:
                        out[:, yo, xo, tap * cin:(tap + 1) * cin] = x[:, yy, xx, :]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# GroupNorm
# ---------------------------------------------------------------------------------------------------------------------
def gn_inputs(seed, B, HW, C, kind="benign", groups=32):
    """x [B, HW, C] bf16 (a different image per batch entry), gamma, beta fp32.
    benign: N(5, 3^2).  pivot0 / pivot1234: N(0, 0.05^2) with one element of every group (its first channel, at pixel 0 or pixel 1234)
    set to 200: at pixel 0 that is the element a first-element pivot would pick."""
    g = gen(seed)
    if kind == "benign":
        x = randn_bf16(g, B, HW, C, scale=3.0, shift=5.0)
    else:
        x = randn_bf16(g, B, HW, C, scale=0.05)
        pix = {"pivot0": 0, "pivot1234": 1234}[kind]
        x[:, pix, ::C // groups] = 200.0
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    return x, gamma, beta


def gn_stats_ref(x, groups=32):
    """(mean, rstd) [B, groups] in float64, population variance, eps 1e-6."""
    B, HW, C = x.shape
    xg = x.to(F64).view(B, HW, groups, C // groups)
    mean = xg.mean((1, 3))
    var = ((xg - mean.view(B, 1, groups, 1)) ** 2).mean((1, 3))
    return mean, (var + 1e-6).rsqrt()


def gn_ref(x, gamma, beta, swish, groups=32):
    """(ref, bound) [B, HW, C] float64 (ref unrounded: the bound's first term is the one bf16 rounding)."""
    B, HW, C = x.shape
    mean, rstd = gn_stats_ref(x, groups)
    cpg = C // groups
    a = rstd.repeat_interleave(cpg, 1) * gamma.to(F64)               # [B, C]
    b = beta.to(F64) - mean.repeat_interleave(cpg, 1) * a
    ax = a.view(B, 1, C) * x.to(F64)
    y = ax + b.view(B, 1, C)
    second = 2.0 ** -16 * (ax.abs() + b.abs().view(B, 1, C))
    if swish:
        y = y * torch.sigmoid(y)
        second = 2 * second
    return y, 2.0 ** -8 * y.abs() + second


def gn_standin(x, gamma, beta, swish, groups=32):
    """fp32 torch group_norm (Welford statistics) on the bf16 input, rounded once."""
    y = F.group_norm(x.float().permute(0, 2, 1), groups, gamma, beta, 1e-6)
    if swish:
        y = y * torch.sigmoid(y)
    return y.permute(0, 2, 1).to(BF16)


def gn_rstd_error(got, x, gamma, beta, groups=32):
    """Largest relative rstd error over the (image, group) pairs, recovered from a swish-less bf16 result: over the elements of a group
    sum(got - beta) * (x - mean) / sum(gamma (x - mean)^2) estimates rstd_kernel, the bf16 output roundings average out."""
    B, HW, C = x.shape
    cpg = C // groups
    mean, rstd = gn_stats_ref(x, groups)
    xc = x.to(F64).view(B, HW, groups, cpg) - mean.view(B, 1, groups, 1)
    num = ((got.to(F64) - beta.to(F64)).view(B, HW, groups, cpg) * xc).sum((1, 3))
    den = (gamma.to(F64).view(1, 1, groups, cpg) * xc * xc).sum((1, 3))
    return ((num / den - rstd).abs() / rstd).max().item()


# ---------------------------------------------------------------------------------------------------------------------
# softmax
# ---------------------------------------------------------------------------------------------------------------------
def softmax_ref(x, scale):
    ref = torch.softmax(x.to(F64) * scale, -1)
    return ref, (2.0 ** -8 + 2.0 ** -14) * ref + 2.0 ** -126


def softmax_standin(x, scale):
    xs = (x - x.max(-1, keepdim=True).values) * scale
    e = torch.exp(xs)
    return (e / e.sum(-1, keepdim=True)).to(BF16)


def softmax_inputs(seed, rows, cols, kind):
    """fp32 scores and the scale they are used with.  normal: N(0, 4^2), scale 0.25.  wide: uniform in +-300, scale 64^-0.5 (the max
    subtraction decides whether exp overflows).  equal: one constant per row, scale 0.25."""
    g = gen(seed)
    if kind == "normal":
        return torch.randn(rows, cols, generator=g) * 4, 0.25
    if kind == "wide":
        return (torch.rand(rows, cols, generator=g) * 2 - 1) * 300, 64 ** -0.5
    if kind == "equal":
        return (torch.randn(rows, 1, generator=g) * 4).expand(rows, cols).contiguous(), 0.25
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------------------------
# reparam
# ---------------------------------------------------------------------------------------------------------------------
REPARAM_SEED = 12          # chosen so that no exp(0.5 logvar) lies within 2^-20 of a bf16 rounding midpoint (test_vae_bf16_ref_cpu.py)
SCALE_FACTOR, SHIFT_FACTOR = 0.3611, 0.1159


def reparam_inputs(seed, n_pix, zc, ld):
    """moments rows [n_pix, ld] bf16 (mean | logvar in the first 2 zc columns, logvar uniform in [-8, 4]), noise [n_pix, zc] bf16."""
    g = gen(seed)
    mom = randn_bf16(g, n_pix, ld)
    mom[:, zc:2 * zc] = (torch.rand(n_pix, zc, generator=g) * 12 - 8).to(BF16)
    noise = randn_bf16(g, n_pix, zc)
    return mom, noise


def reparam_ref(mom, noise, zc, scale=SCALE_FACTOR, shift=SHIFT_FACTOR):
    """Eager bf16 torch, op for op what DiagonalGaussian.sample and the latent scaling do under autocast: exp(0.5 logvar),
    mean + std noise, scale (z - shift), every op rounding its result to bf16.

    One op is written out.  On the device a python scalar enters a bf16 elementwise op as an fp32 operand (the op computes in fp32 and
    rounds once), and the kernel follows that.  The CPU backend does the same for ``scale * t`` but rounds the scalar of ``z - shift`` to
    bf16 first (0.1159 -> 0.11572...), which moves about one result in ten by a bf16 ulp; so the subtraction is spelled as the fp32
    operation it is on the device.  test_vae_bf16_ref_cpu.py pins both facts and test_vae_bf16_gpu.py checks this reference against
    eager bf16 torch on the device."""
    mean, logvar = mom[:, :zc], mom[:, zc:2 * zc]
    assert mean.dtype == BF16
    if noise is None:
        z = mean
    else:
        std = torch.exp(0.5 * logvar)
        z = mean + std * noise
    assert z.dtype == BF16
    return scale * (z.float() - shift).to(BF16)


def reparam_eager(mom, noise, zc, scale=SCALE_FACTOR, shift=SHIFT_FACTOR):
    """The literal eager expression, on whatever device the operands live."""
    mean, logvar = mom[:, :zc], mom[:, zc:2 * zc]
    z = mean if noise is None else mean + torch.exp(0.5 * logvar) * noise
    return scale * (z - shift)


def reparam_emulated(mom, noise, zc, scale=SCALE_FACTOR, shift=SHIFT_FACTOR):
    """The same with every rounding written out in fp32 (the formula of vae_reparam_bf16_kernel): python scalars stay fp32."""
    def r(v):
        return v.to(BF16).float()
    mean, logvar = mom[:, :zc].float(), mom[:, zc:2 * zc].float()
    s = mean
    if noise is not None:
        std = r(torch.exp(r(0.5 * logvar)))
        s = r(mean + r(std * noise.float()))
    return (torch.tensor(scale, dtype=torch.float32) * r(s - torch.tensor(shift, dtype=torch.float32))).to(BF16)


def reparam_exp_midpoint_margin(mom, zc):
    """Smallest relative distance between a float64 exp(0.5 logvar) and the nearest bf16 rounding midpoint."""
    e = torch.exp(0.5 * mom[:, zc:2 * zc].to(F64))
    m, ex = torch.frexp(e)                      # e = m 2^ex, m in [0.5, 1): bf16 spacing 2^-8 in m, midpoints at odd multiples of 2^-9
    q = m * 2.0 ** 9
    odd = torch.floor((q - 1) / 2 + 0.5) * 2 + 1          # nearest odd integer
    return ((q - odd).abs() / q).min().item()


# ---------------------------------------------------------------------------------------------------------------------
# attention block, float64 with the engine's cast points
# ---------------------------------------------------------------------------------------------------------------------
def attn_block_ref(x, m):
    """x [B, H, W, C] bf16; m the AttnBlock (fp32 parameters, on the CPU).  Cast points of VaeEngineBf16.attn: bf16 GroupNorm result,
    bf16 q / k / v (bf16 weights and bias), fp32 scores, bf16 probabilities, bf16 P V, bf16(bf16(proj + bias) + x)."""
    B, H, W, C = x.shape
    N = H * W
    xs = x.view(B, N, C)
    h = rbf(gn_ref(xs, m.norm.weight.data, m.norm.bias.data, False)[0])

    def lin(v, c):
        w = c.weight.data.reshape(C, C).to(BF16).to(F64)
        return v @ w.t() + c.bias.data.to(BF16).to(F64)
    q, k, v = rbf(lin(h, m.q)), rbf(lin(h, m.k)), rbf(lin(h, m.v))
    p = rbf(torch.softmax((q @ k.transpose(1, 2)) * float(C) ** -0.5, -1))
    o = rbf(p @ v)
    return rbf(rbf(lin(o, m.proj_out)) + xs.to(F64)).view(B, H, W, C)


def chained_check(got, ref, ulps=2.0, rel_l2=4e-3):
    """(max|d| / allowed, rel-L2 / allowed) under the SURVEY.md 8c convention."""
    got, ref = got.to(F64), ref.to(F64)
    assert got.shape == ref.shape
    if not torch.isfinite(got).all():
        return float("inf"), float("inf")
    d = (got - ref).abs().max().item() / (ulps * 2.0 ** -7 * ref.abs().max().item())
    l2 = ((got - ref).norm() / ref.norm()).item() / rel_l2
    return d, l2


# ---------------------------------------------------------------------------------------------------------------------
# the cases, shared by the GPU tests and the CPU validation of the bounds
# ---------------------------------------------------------------------------------------------------------------------
CONV_CASES = [(8, 136, 9, 13), (24, 40, 9, 13), (64, 3, 16, 16), (64, 6, 9, 13), (128, 260, 6, 10), (160, 8, 6, 10)]   # Cin, Cout, H, W
# M, N, K, fp32 output, pad elements on the input rows (ld_in = K + pad), pad elements on the output rows
GEMM_CASES = [(1, 8, 8, False, 0, 0), (6, 7, 8, True, 8, 5), (130, 64, 72, False, 8, 8), (300, 132, 240, False, 16, 4),
              (35, 40, 40, True, 0, 4)]
GN_SHAPES = [(C, HW) for C in (64, 128, 512, 96, 160) for HW in (16, 240, 130)] + [(64, 6401), (96, 6401)]
GN_OUTLIER_CASES = [(64, "pivot0"), (96, "pivot0"), (64, "pivot1234"), (96, "pivot1234")]
GN_OUTLIER_HW = 37 * 173
SOFTMAX_COLS = [1, 5, 255, 256, 257, 1000, 4099]
REPARAM_CASES = [(16, 32), (4, 16)]          # z_channels, ld_moments
N_PIX = 256


def conv_variants(cout):
    """(bias, residual) combinations of one random conv case."""
    return [(True, False), (False, False)] + ([(True, True)] if cout % 8 == 0 else [])


def conv_seed(mode, cin, cout):
    return 1000 * mode + cin + cout
