"""Float64 reference, per-element checks, designed input families and an fp32 emulation (+ wrong variants) of the matrix products
C = A W^T (+ bias)(activation)(+ residual): gemm.hip (tile, ping-pong, persistent, K-split reduce), skinny.hip, the lane-FMA gemv of
decode.hip, gemv_mb.hip and the fp8 form of the persistent kernel.  Pure torch on the CPU; tests/test_gemm_ref_cpu.py validates it,
tests/test_gemm_designed_gpu.py applies it to the HIP kernels.

THE ROUNDING SEQUENCE (``acc`` = the fp32 sum over k, fp8: times the fp32 product sa[row] * sw[n]; every kernel spells the same one)

    o = acc + bias                   fp32          gemm.hip `o[0] += lo2f(bv[0])` (tile), `o[0] += lo2f(bv[nb][jn][0])` (persistent),
                                                   gemm_splitk_reduce_kernel `o[0] += lo2f(bv[0])`; skinny.hip / gemv_mb.hip the same line;
                                                   decode.hip `if (p.bias) o[t] += eb[t]`
    o = act(bf16(o))                 GELU / SiLU   `o[e] = gelu_tanh_f(bfround(o[e]))`, `o[e] = silu_f(bfround(o[e]))` in all of them
    c1 = bf16(o)                                   `pack2bf(o[0], o[1])`; with a residual `bfround(o[0]) + lo2f(rv[0])` (tile, skinny, gemv_mb),
                                                   decode.hip `if (p.R) o[t] = bfround(o[t]) + er[m][t]`
    out = bf16(c1 + r)               fp32 sum      the same lines; ping-pong / persistent / reduce: `pack2bf(lo2f(v[0]) + lo2f(rv[0]), ..)`
                                                   on the packed c1
    SwiGLU16 (no bias, no residual): columns in blocks of 32 = 16 gate then 16 up columns; out[m, 16 b + j] =
        bf16(bf16(silu(bf16(acc_gate))) * bf16(acc_up))      `o[e] = bfround(silu_f(g)) * u` on `g = bfround(acc..)`, `u = bfround(acc..)`
  The tile, ping-pong, persistent, reduce, skinny, gemv and gemv_mb epilogues were read side by side for this module: none rounds at
  another point, so exact inputs must give the same bits on every path.

THE BOUND  (u = 2^-8: bf16 unit roundoff; eps = 2^-24; S = sum_k |a||w| + |bias|; t = the float64 value of acc + bias)

    no residual      |got - t| <= u |t| + c S,    c = 2 (K + 2) eps
        products of two bf16 are exact in fp32; K - 1 additions of the sum in ANY order (k-tiles, MFMA blocks, K parts, wave reductions)
        and one for the bias: each partial sum is bounded by S, so the error is <= K eps' S to first order; + 2 covers the second-order
        terms ((1 + eps')^K - 1 - K eps' < 2 eps' for K <= 2^17).  eps' = 2 eps: the MFMA accumulate may truncate instead of rounding
        (MI355X_MICROARCH.md gives no rounding mode for the matrix pipe's internal adds; the lane-FMA gemv rounds to nearest and needs half).
    residual r       |got - (t + r)| <= u |t| + u (|t + r| + u |t|) + c S        AND membership: got = bf16(c1 + r) for some bf16 c1 with
                     |c1 - t| <= u |t| + c S  (a merged rounding bf16(t + r) satisfies the first line and fails the second)
    GELU / SiLU      |got - act(t)| <= u |act(t)| + L (u |t| + c S)  [+ |t| 2^-22 for GELU]
        u |act|: the output rounding (u / 2) + the fp32 evaluation; L = sup |act'| (GELU-tanh 1.13, SiLU 1.10) carries the input's bound;
        The GELU term widens the issue's rule, from common.h gelu_tanh_f `return 0.5f * x * (1.0f + tanhf(inner));`: for x < 0 the fp32 sum
        1.0f + tanhf(inner) cancels, and what is left carries the absolute error of its operands, a few ulp of 1 (tanhf: <= 2 ulp, the sum's
        rounding 1/2 ulp; ulp(1) = 2^-23), not of the small result.  Times 0.5 |x| that is <= 4 * 2^-24 |x| = |x| 2^-22 in absolute terms, which
        u |act(x)| does not cover once |act(x)| < 2^-14 |x| (x below about -4).
    SwiGLU           s = silu(g): |s~ - s| <= bs = u |s| + L bg;  |u~ - up| <= bu;  |got - s up| <= u |s up| + (1 + u)(bs |up| + bu |s| + bs bu)
  ``exact_input=True`` (families whose accumulator is exact): bg = bu = 0 and the activation's input is the one bf16(t), so the output
  is within u |act(bf16 t)| of it -- that is what rejects an activation taken of the unrounded value.
  Results below 2^-116 (fp32 / bf16 share the exponent range; `__expf` overflows past 88) are compared with that absolute floor.

FAMILIES (seeded; each asserts its own precondition)
  exact       A dense +-1, W in {-1, 0, +1} (density ~900 / K), integer bias / residual: every partial sum in any order is an integer
              <= 256, exact in fp32 and in bf16 -> ONE legal bit pattern.
  kprobe      A[m, :] = indicator of [0, j(m)), j over every multiple of 8 up to K; W = +-1 with |prefix sums| <= 64: C is a prefix sum.
  roundpoint  acc = sigma_m T_n exact, T_n a multiple of 1/4 in [128, 256) (ulp 1), bias multiples of 1/2, residual of 1/4 (all times
              ``scale``, a power of two): rounding after the bias and again after the residual / one merged rounding / bias after the
              rounding differ on >= 1/4 of the elements, ties occur.
  scaled      real values; row scales of A and of W span 2^-8 .. 2^8 (``small_rows`` at 2^-8: the MoT marker rows).
  cancel      S >= 2^10 |t|: the second half of K holds the negated, slightly perturbed copy of the first.
  edges       real values in buffers larger than the problem: NaN in the A rows no list entry names, sentinels in every C element that
              must not be written.

EMULATION  ``emulate`` restates the schedule in fp32 torch: 64-deep k-tiles, a K tail that reads zeros, K parts [nk p / s, nk (p + 1) / s),
an fp32 reduce in part order, the rounding sequence above; ``MUTANTS`` are the ways it can be subtly wrong.
"""
import math

import torch

BF16 = torch.bfloat16
F64 = torch.float64
EPS = 2.0 ** -24
U = 2.0 ** -8
TINY = 2.0 ** -116
EPI_NONE, EPI_GELU, EPI_SILU, EPI_SWIGLU = 0, 1, 2, 3
LIP = {EPI_GELU: 1.13, EPI_SILU: 1.10}
SENTINEL = -1232.0          # exact in bf16; no family produces it


def cbound(K):
    return 2.0 * (K + 2) * EPS


def bits(x):
    return x.contiguous().view(torch.int16)


def rne(x64):
    """float64 -> bf16, round to nearest even (one rounding: callers pass values that fp32 holds exactly, or accept the double rounding)."""
    return x64.to(torch.float32).to(BF16)


def act64(x, epi):
    if epi == EPI_GELU:
        return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)))
    if epi == EPI_SILU:
        return x * torch.sigmoid(x)
    return x


def bf16_step(x, k):
    """The bf16 value k representable steps above x (k may be negative); x bf16, finite."""
    b = bits(x).to(torch.int32) & 0xFFFF
    o = torch.where(b >= 0x8000, -(b & 0x7FFF), b) + k
    nb = torch.where(o < 0, (-o) | 0x8000, o)
    nb = torch.where(nb >= 0x8000, nb - 0x10000, nb).to(torch.int16)
    return nb.view(BF16)


# ------------------------------------------------------------------------------------------------------------
# a problem in the layout of ops.gemm
# ------------------------------------------------------------------------------------------------------------
class Case:
    """A [Ma, K] bf16 (rows no group names may hold NaN), up to two row groups {W [N, K], bias [N] | None, a_rows / c_rows (list | None),
    M}, epilogue, C0 [Mc, ldc] the initial C buffer: the residual (``res``: added in place) where a group writes, NaN there otherwise,
    SENTINEL wherever nothing may be written."""

    def __init__(self, name, A, groups, epi=EPI_NONE, res=False, C0=None, exact=False, scale=1.0):
        self.name, self.A, self.groups, self.epi, self.res, self.exact, self.scale = name, A, groups, epi, res, exact, scale
        self.N, self.K = groups[0]["W"].shape
        self.Nout = self.N // 2 if epi == EPI_SWIGLU else self.N
        self.C0 = C0
        self.written = torch.zeros(C0.shape, dtype=torch.bool)
        for g in groups:
            self.written[self.crows(g), :self.Nout] = True
        assert int(self.written.sum()) == sum(g["M"] for g in groups) * self.Nout, "c_rows overlap"
        assert res or bool(torch.isnan(C0[self.written].float()).all())
        assert bool((C0[~self.written].float() == SENTINEL).all())

    @staticmethod
    def arows(g):
        return torch.arange(g["M"]) if g["a_rows"] is None else torch.tensor(g["a_rows"], dtype=torch.long)

    @staticmethod
    def crows(g):
        return torch.arange(g["M"]) if g["c_rows"] is None else torch.tensor(g["c_rows"], dtype=torch.long)


def reference(case):
    """-> dict of float64 [Mc, N] arrays over the physical C rows: t = A W^T + bias, S = |A||W|^T + |bias|, r [Mc, Nout] (the residual)."""
    Mc = case.C0.shape[0]
    t, S = torch.zeros(Mc, case.N, dtype=F64), torch.zeros(Mc, case.N, dtype=F64)
    for g in case.groups:
        a = case.A[case.arows(g)].to(F64)
        assert bool(torch.isfinite(a).all()), "a row list names a NaN row"
        w = g["W"].to(F64)
        tt, ss = a @ w.t(), a.abs() @ w.abs().t()
        if g["bias"] is not None:
            tt, ss = tt + g["bias"].to(F64), ss + g["bias"].to(F64).abs()
        t[case.crows(g)], S[case.crows(g)] = tt, ss
    r = case.C0[:, :case.Nout].to(F64) if case.res else None
    return dict(t=t, S=S, r=r)


def _pair(x):
    """[M, N] -> (gate, up) [M, N / 2]: 16-column blocks, gate block then up block."""
    v = x.view(x.shape[0], -1, 2, 16)
    return v[:, :, 0].reshape(x.shape[0], -1), v[:, :, 1].reshape(x.shape[0], -1)


def expected_bits(case, ref):
    """The one legal result of an exact-accumulator case without activation: bf16 [Mc, Nout]."""
    assert case.exact and case.epi == EPI_NONE
    c1 = rne(ref["t"])
    assert bool((ref["t"].to(torch.float32).to(F64) == ref["t"]).all()), "exact family: acc + bias is not exact in fp32"
    if case.res:
        c1 = (c1.float() + case.C0[:, :case.Nout].float()).to(BF16)
    return c1


def _where(case, idx):
    m, n = divmod(int(idx), case.Nout)
    return f"physical C row {m}, column {n} (256-tile ({m // 256}, {n // 256}), 128-tile ({m // 128}, {n // 128}))"


def assert_untouched(case, got, what=""):
    same = bits(got) == bits(case.C0)
    bad = ~same & ~case.written
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        m, n = divmod(i, case.C0.shape[1])
        raise AssertionError(f"{what} {case.name}: sentinel at C[{m}, {n}] was overwritten with {got[m, n].item()} ({int(bad.sum())} elements)")


def ratio(case, got, ref, exact_input=None):
    """Worst err / bound over the written elements (NaN / Inf output -> inf), its flat index in [Mc, Nout], and the membership verdict."""
    exact_input = case.exact if exact_input is None else exact_input
    K, epi = case.K, case.epi
    c = 0.0 if exact_input else cbound(K)
    t, S = ref["t"], ref["S"]
    g64 = got[:, :case.Nout].to(F64)
    member = None
    if epi == EPI_SWIGLU:
        (tg, tu), (Sg, Su) = _pair(t), _pair(S)
        if exact_input:
            tg, tu = rne(tg).to(F64), rne(tu).to(F64)
        s = act64(tg, EPI_SILU)
        bg, bu = (0.0, 0.0) if exact_input else (U * tg.abs() + c * Sg, U * tu.abs() + c * Su)
        bs = U * s.abs() + LIP[EPI_SILU] * bg + TINY
        want = s * tu
        bound = U * want.abs() + (1 + U) * (bs * tu.abs() + bu * s.abs() + bs * bu) + TINY
    elif epi in (EPI_GELU, EPI_SILU):
        assert not case.res, "activation + residual is not served by this reference"
        x = rne(t).to(F64) if exact_input else t
        want = act64(x, epi)
        bin_ = 0.0 if exact_input else U * t.abs() + c * S
        bound = U * want.abs() + LIP[epi] * bin_ + TINY + (x.abs() * 2.0 ** -22 if epi == EPI_GELU else 0.0)
    elif case.res:
        r = ref["r"]
        b1 = U * t.abs() + c * S
        want = t + r
        bound = b1 + U * (want.abs() + U * t.abs())
        member = _member(got[:, :case.Nout], t, b1, case.C0[:, :case.Nout])
    else:
        want, bound = t, U * t.abs() + c * S
    err = (g64 - want).abs()
    q = err / bound.clamp_min(1e-300)
    q = torch.where(torch.isfinite(g64), q, torch.full_like(q, float("inf")))
    q = torch.where(err == 0, torch.zeros_like(q), q)
    w = case.written[:, :case.Nout]
    q = torch.where(w, q, torch.zeros_like(q))
    if member is not None:
        member = bool((member | ~w).all())
    i = int(q.argmax())
    return float(q.flatten()[i]), i, member


def _member(got, t, b1, r):
    """got == bf16(c1 + r) (the kernels' fp32 sum, then one rounding) for a bf16 c1 with |c1 - t| <= b1 ?  Elementwise bool."""
    gp, gn = bf16_step(got, -1).to(F64), bf16_step(got, 1).to(F64)
    lo2 = (got.to(F64) + gp) / 2 - r.to(F64)                       # c1 + r rounds to got only above this midpoint
    lo = torch.maximum(t - b1, lo2)
    start = rne(lo)                                               # a bf16 next to the lower end of the candidates: try its neighbours
    ok = torch.zeros(got.shape, dtype=torch.bool)
    for k in (-1, 0, 1, 2):
        c1 = bf16_step(start, k)
        valid = (c1.to(F64) - t).abs() <= b1
        ok |= valid & (bits((c1.float() + r.float()).to(BF16)) == bits(got))
    return ok | (gn != gn)


def assert_case(case, got, ref=None, what="", bitwise=None):
    """got: the whole C buffer [Mc, ldc] after the call.  Exact-accumulator cases without activation: the one legal bit pattern;
    everything else: the per-element bound (+ membership with a residual).  No sentinel may change.  -> worst err / bound (0.0: exact)."""
    ref = reference(case) if ref is None else ref
    assert got.shape == case.C0.shape and got.dtype == BF16
    assert_untouched(case, got, what)
    bitwise = (case.exact and case.epi == EPI_NONE) if bitwise is None else bitwise
    w = case.written[:, :case.Nout]
    if bitwise:
        exp = expected_bits(case, ref)
        bad = (bits(got[:, :case.Nout]) != bits(exp)) & w
        # -0 / +0: an exact zero may carry either sign of the last addend
        bad &= ~((got[:, :case.Nout].float() == 0) & (exp.float() == 0))
        if bool(bad.any()):
            i = int(bad.flatten().nonzero()[0])
            m, n = divmod(i, case.Nout)
            raise AssertionError(f"{what} {case.name}: {int(bad.sum())} of {int(w.sum())} elements differ from the exact result; first at {_where(case, i)}: "
                                 f"got {got[m, n].item()} expected {exp[m, n].item()} (t = {ref['t'][m, n].item()})")
        return 0.0
    q, i, member = ratio(case, got, ref)
    if q > 1.0 or member is False:
        m, n = divmod(i, case.Nout)
        if case.epi == EPI_SWIGLU:                                    # output column n pairs the gate column 32 (n / 16) + n % 16 with the up column 16 further on
            ng = 32 * (n // 16) + n % 16
            tval = f"t(gate, column {ng}) = {ref['t'][m, ng].item()}, t(up, column {ng + 16}) = {ref['t'][m, ng + 16].item()}"
        else:
            tval = f"t = {ref['t'][m, n].item()}"
        raise AssertionError(f"{what} {case.name}: err / bound = {q:.3f} at {_where(case, i)}: got {got[m, n].item()}, {tval}"
                             f"{'' if member is not False else '; some element is no two-rounding result bf16(bf16(t) + r)'}")
    return q


# ------------------------------------------------------------------------------------------------------------
# designed families: dense parts (A [M, K], W [N, K], bias [N], R [M, N]) as bf16 tensors
# ------------------------------------------------------------------------------------------------------------
def _gen(*seed):
    s = 0
    for x in seed:
        s = (s * 1000003 + int(x) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _signs(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).to(torch.float32)


def fam_exact(M, N, K, seed=0, wseed=0):
    ga, gw = _gen(1, seed, M, K), _gen(2, seed, wseed, N, K)
    A = _signs((M, K), ga)
    dens = min(1.0, 900.0 / K)
    W = _signs((N, K), gw) * (torch.rand((N, K), generator=gw) < dens)
    bias = torch.randint(-20, 21, (N,), generator=gw).float()
    R = torch.randint(-60, 61, (M, N), generator=_gen(3, seed, M, N)).float()
    t = A.double() @ W.double().t()
    lim = float(t.abs().max()) + 20 + 60
    assert lim <= 256 and float((A.double().abs() @ W.double().abs().t()).max()) <= 2 ** 24, f"exact: |C| + |bias| + |r| reaches {lim}"
    return dict(A=A.to(BF16), W=W.to(BF16), bias=bias.to(BF16), R=R.to(BF16))


def fam_kprobe(M, N, K, seed=0, wseed=0):
    gw = _gen(4, seed, wseed, N, K)
    nj = K // 8 + 1
    if M >= nj:
        j = 8 * (torch.arange(M) % nj)                               # every multiple of 8 in [0, K]
    else:
        j = 8 * torch.linspace(0, nj - 1, M).round().long() if M > 1 else torch.tensor([K])      # fewer rows: evenly spread, the last one all of K
    A = (torch.arange(K)[None, :] < j[:, None]).float()
    steps = _signs((N, K), gw)
    W = torch.empty(N, K)
    pre = torch.zeros(N)
    for k in range(K):                                               # a walk reflected at +-64
        s = torch.where((pre + steps[:, k]).abs() > 64, -steps[:, k], steps[:, k])
        W[:, k] = s
        pre = pre + s
    assert float(W.cumsum(1).abs().max()) <= 64
    bias = torch.randint(-20, 21, (N,), generator=gw).float()
    R = torch.randint(-60, 61, (M, N), generator=_gen(5, seed, M, N)).float()
    return dict(A=A.to(BF16), W=W.to(BF16), bias=bias.to(BF16), R=R.to(BF16))


def fam_roundpoint(M, N, K, seed=0, wseed=0, scale=1.0):
    gs, gw = _gen(6, seed, K), _gen(7, seed, wseed, N, K)
    sk = _signs((K,), gs)
    sm = _signs((M,), _gen(8, seed, M))
    # T_n in quarter units.  Three columns of four: T = k + 1/4 or k + 3/4 with a half-odd bias (T + b sits a quarter off an integer, bf16(T) + b on a
    # tie); the fourth: T = k + 1/2 with an odd integer bias (a tie whose even neighbour the bias flips)
    cls_b = torch.arange(N) % 4 == 3
    q = torch.randint(128, 255, (N,), generator=gw) * 4 + torch.where(cls_b, 2, 1 + 2 * torch.randint(0, 2, (N,), generator=gw))
    base, rem = q // K, q % K
    assert int(base.max()) + 9 <= 255, "roundpoint: K too short for 8-bit quarter units"
    e = base[:, None].repeat(1, K) + (torch.arange(K)[None, :] < rem[:, None]).long()
    d = torch.randint(0, 9, (N, K // 2), generator=gw)
    d = torch.minimum(d, torch.minimum(e[:, 0:2 * (K // 2):2], e[:, 1:2 * (K // 2):2]))
    e[:, 0:2 * (K // 2):2] += d
    e[:, 1:2 * (K // 2):2] -= d
    e = torch.gather(e, 1, torch.rand((N, K), generator=gw).argsort(1))   # the quarter units spread over all of K
    assert int(e.min()) >= 0 and int(e.max()) <= 255 and bool((e.sum(1) == q).all())
    W = e.float() / 4 * sk[None, :] * scale
    A = sm[:, None] * sk[None, :].repeat(M, 1)
    h = 2 * torch.randint(-4, 4, (N,), generator=gw) + 1               # odd, in half units
    bias = (torch.where(cls_b, 2 * (h // 2 * 2 + 1), h).float() / 2) * scale
    gr = _gen(9, seed, M, N)
    frac = torch.tensor([2, 2, 1, 3])[torch.randint(0, 4, (M, N), generator=gr)]          # residual: a half twice as often as one or three quarters
    R = ((4 * torch.randint(-7, 8, (M, N), generator=gr) + frac).float() / 4) * scale
    p = dict(A=A.to(BF16), W=W.to(BF16), bias=bias.to(BF16), R=R.to(BF16))
    assert all(bool((p[k].float() == v).all()) for k, v in (("A", A), ("W", W), ("bias", bias), ("R", R)))
    acc = A.double() @ W.double().t()
    assert bool((acc.abs() >= 128 * scale).all()) and bool((acc.abs() < 256 * scale).all())
    # the three rounding sequences must disagree, and ties must occur
    b, r = bias.double(), R.double()
    two = rne(rne(acc + b).double() + r)
    merged = rne(acc + b + r)
    after = rne(rne(rne(acc).double() + b).double() + r)
    after_nores = rne(rne(acc).double() + b)
    f1, f2, f3 = [float((bits(two) != bits(x)).float().mean()) for x in (merged, after)] + [float((bits(rne(acc + b)) != bits(after_nores)).float().mean())]
    few = M * N < 256                                                 # the shares are statistics: a handful of elements (M = 1, N = 6) cannot be held to them
    assert few or min(f1, f2, f3) >= 0.25, f"roundpoint: the rounding sequences differ on only {f1:.2f} / {f2:.2f} / {f3:.2f} of the elements"
    ulp = scale                                                       # bf16 spacing in [128, 256) * scale
    x1 = (acc + b) / ulp
    x2 = (rne(acc + b).double() + r) / ulp
    ties = float((((x1 - x1.floor()) == 0.5) | ((x2 - x2.floor()) == 0.5)).float().mean())
    assert few or ties >= 0.2, f"roundpoint: only {ties:.2f} of the elements meet a tie"
    return p


def fam_scaled(M, N, K, seed=0, wseed=0, small_rows=(), span=8.0):
    ga, gw = _gen(10, seed, M, K), _gen(11, seed, wseed, N, K)
    ra = 2.0 ** ((torch.rand(M, generator=ga) * 2 - 1) * span)
    if M >= 2:
        ra[0], ra[1 if M >= 3 else M - 1] = 2.0 ** -span, 2.0 ** span
    for i in small_rows:
        ra[i] = 2.0 ** -span
    rw = 2.0 ** ((torch.rand(N, generator=gw) * 2 - 1) * span)
    rw[0], rw[N - 1] = 2.0 ** span, 2.0 ** -span
    A = torch.randn(M, K, generator=ga) * ra[:, None]
    W = torch.randn(N, K, generator=gw) * K ** -0.5 * rw[:, None]
    bias = torch.randn(N, generator=gw) * 0.3 * rw
    R = torch.randn(M, N, generator=_gen(12, seed, M, N)) * ra[:, None] * rw[None, :]
    p = dict(A=A.to(BF16), W=W.to(BF16), bias=bias.to(BF16), R=R.to(BF16))
    rms = p["A"].float().pow(2).mean(1).sqrt()
    assert M < 2 or float(rms.max() / rms.min()) >= 2.0 ** (2 * span - 2), "scaled: the row scales do not span the range"
    return p


def fam_cancel(M, N, K, seed=0, wseed=0):
    assert K % 2 == 0
    ga, gw = _gen(13, seed, M, K), _gen(14, seed, wseed, N, K)
    h = K // 2
    x = torch.randn(M, h, generator=ga).to(BF16)
    w = (torch.randn(N, h, generator=gw) * K ** -0.5).to(BF16)
    flip = torch.rand((N, h), generator=gw) < 1.0 / 16                # the perturbation: one bf16 step on 1/16 of the copy
    w2 = torch.where(flip, bf16_step(w, 1), w)
    A = torch.cat([x, x], 1)
    W = torch.cat([w, -w2], 1)
    bias = torch.zeros(N)
    R = (torch.randn(M, N, generator=_gen(15, seed, M, N)) * 2.0 ** -6).to(BF16)
    t = A.double() @ W.double().t()
    S = A.double().abs() @ W.double().abs().t()
    share = float((S >= 2 ** 10 * t.abs()).float().mean())
    assert M * N < 256 or share >= 0.9, f"cancel: only {share:.2f} of the elements cancel by 2^10"
    return dict(A=A, W=W, bias=bias.to(BF16), R=R)


FAMILIES = {"exact": fam_exact, "kprobe": fam_kprobe, "roundpoint": fam_roundpoint, "scaled": fam_scaled, "cancel": fam_cancel, "edges": fam_scaled}
EXACT_FAMILIES = ("exact", "kprobe", "roundpoint")
EPILOGUES = ("plain", "bias", "res", "bias_res", "bias_gelu", "silu", "swiglu", "groups", "gather")


def marker_rows(M):
    """Rows of a packed MoT batch: samples of [<start>, latents.., <end>]; -> (marker rows, latent rows)."""
    ns = min(4, M // 3)
    if ns == 0:
        return list(range(M)), []
    lens = [M // ns] * ns
    lens[-1] += M - sum(lens)
    rt, rv, base = [], [], 0
    for n in lens:
        rt += [base, base + n - 1]
        rv += list(range(base + 1, base + n - 1))
        base += n
    return rt, rv


def build(family, M, N, K, epi="plain", seed=0, scale=None):
    """One problem of ``family`` with the epilogue / routing ``epi`` (EPILOGUES).  ``edges`` pads every buffer; the other families use
    tight ones (C rows and columns exactly the problem's)."""
    pad = family == "edges"
    fam = FAMILIES[family]
    kw = {}
    if family == "roundpoint":
        kw["scale"] = (2.0 ** -7 if epi in ("bias_gelu", "silu", "swiglu") else 1.0) if scale is None else scale
    if family == "edges":
        kw["span"] = 2.0
    rt, rv = marker_rows(M) if epi == "groups" else (None, None)
    if family == "scaled" and epi == "groups":
        kw["small_rows"] = rt
    p0 = fam(M, N, K, seed=seed, wseed=0, **kw)
    A, R = p0["A"], p0["R"]
    e = {"bias_gelu": EPI_GELU, "silu": EPI_SILU, "swiglu": EPI_SWIGLU}.get(epi, EPI_NONE)
    has_bias = epi in ("bias", "bias_res", "bias_gelu", "groups", "gather")
    res = epi in ("res", "bias_res", "groups")
    Nout = N // 2 if e == EPI_SWIGLU else N
    if epi == "groups":
        p1 = fam(M, N, K, seed=seed, wseed=1, **kw)
        assert torch.equal(bits(p1["A"]), bits(A))
        glist = [(p0, rt), (p1, rv)]
        logical = [(r, r) for _, r in glist]
    elif epi == "gather":
        rows = [i for i in range(M) if i % 7 != 3] if M > 1 else [0]
        glist = [(p0, rows)]
        logical = [(rows, list(range(len(rows))))]                    # gathered A rows -> dense C rows
    else:
        glist = [(p0, None)]
        logical = [(None, None)]
    # physical layout
    Mc_log = len(logical[0][0]) if epi == "gather" else M
    spread = (lambda i: 2 * i + 1) if pad else (lambda i: i)
    Ma = (2 * M + 3) if pad else M
    Mc = (2 * Mc_log + 3) if pad else Mc_log
    ldc = Nout + 8 if pad else Nout
    Abuf = torch.full((Ma, K), float("nan"), dtype=BF16)
    C0 = torch.full((Mc, ldc), SENTINEL, dtype=BF16)
    if pad and epi not in ("groups", "gather"):                       # dense: rows [0, M) + NaN / sentinel rows beyond
        spread = lambda i: i                                          # noqa: E731
    Abuf[[spread(i) for i in range(M)]] = A
    groups = []
    for (p, _), (ar, cr) in zip(glist, logical):
        Mg = M if ar is None else len(ar)
        if Mg == 0:
            continue
        a_rows = None if ar is None else [spread(i) for i in ar]
        c_rows = None if cr is None else [spread(i) for i in cr]
        if epi == "gather" and not pad:
            c_rows = None
        groups.append(dict(W=p["W"], bias=p["bias"] if has_bias else None, a_rows=a_rows, c_rows=c_rows, M=Mg))
        crow = torch.arange(Mg) if c_rows is None else torch.tensor(c_rows)
        src = torch.arange(Mg) if cr is None else torch.tensor(cr)
        C0[crow, :Nout] = R[src][:, :Nout] if res else torch.full((Mg, Nout), float("nan"), dtype=BF16)
    exact = family in EXACT_FAMILIES
    return Case(f"{family}/{epi} {M}x{N}x{K}", Abuf, groups, epi=e, res=res, C0=C0, exact=exact, scale=kw.get("scale", 1.0))


# ------------------------------------------------------------------------------------------------------------
# fp32 emulation of the schedule, and the ways to get it wrong
# ------------------------------------------------------------------------------------------------------------
MUTANTS = ("drop_chunk_ktile", "double_chunk_ktile", "drop_chunk_ksplit", "double_chunk_ksplit", "parts_off_by_one", "ktail_not_zeroed",
           "partials_bf16", "bias_after_rounding", "merged_residual", "gelu_unrounded", "clamp_dup", "bias_chunk_prev", "swiglu_swap",
           "wrong_group_weight", "crows_off_by_one", "stale_lds_chunk")


def _bf(x):
    return x.to(BF16).to(torch.float32)


def _act32(x, epi):
    if epi == EPI_GELU:
        return torch.nn.functional.gelu(x, approximate="tanh")
    return torch.nn.functional.silu(x)


def emulate(case, split=1, mutant=None):
    """-> the C buffer [Mc, ldc] bf16 an honest (mutant=None) kernel with this schedule leaves."""
    K, N, Nout = case.K, case.N, case.Nout
    nk = (K + 63) // 64
    Kp = nk * 64
    s = max(1, min(split, nk))
    C = case.C0.clone()
    for gi, g in enumerate(case.groups):
        ar = case.arows(g)
        a = case.A[ar].float()
        Wg = g["W"]
        if mutant == "wrong_group_weight" and gi == 0 and len(case.groups) > 1:
            Wg = case.groups[1]["W"]
        w = Wg.float()
        ap, wp = torch.zeros(g["M"], Kp), torch.zeros(N, Kp)
        ap[:, :K], wp[:, :K] = a, w
        if mutant == "ktail_not_zeroed" and Kp > K:                   # the chunks past K: the start of the next row in memory
            ap[:, K:] = torch.roll(a, -1, 0)[:, :Kp - K]
            wp[:, K:] = torch.roll(w, -1, 0)[:, :Kp - K]
        kb = 64 * (nk // s) if s > 1 else 64                          # first chunk of K part 1 / of k-tile 1
        if mutant in ("drop_chunk_ktile", "double_chunk_ktile") and nk > 1:
            ap[:, 64:72] *= 0.0 if mutant.startswith("drop") else 2.0
        if mutant in ("drop_chunk_ksplit", "double_chunk_ksplit") and s > 1:
            ap[:, kb:kb + 8] *= 0.0 if mutant.startswith("drop") else 2.0
        if mutant == "stale_lds_chunk" and nk > 1:                    # one tile row, k-tile 1, chunk 3: still the previous k-tile's bytes
            m = min(5, g["M"] - 1)
            ap[m, 64 + 24:64 + 32] = ap[m, 24:32]
        parts = []
        for p in range(s):
            t0, t1 = nk * p // s, nk * (p + 1) // s
            if mutant == "parts_off_by_one" and s > 1 and p == 0:
                t1 -= 1
            acc = torch.zeros(g["M"], N)
            for kt in range(t0, t1):
                acc = acc + ap[:, 64 * kt:64 * kt + 64] @ wp[:, 64 * kt:64 * kt + 64].t()
            parts.append(_bf(acc) if mutant == "partials_bf16" and s > 1 else acc)
        acc = parts[0]
        for x in parts[1:]:
            acc = acc + x
        cr = case.crows(g)
        if mutant == "crows_off_by_one" and g["c_rows"] is not None and g["M"] > 1:
            cr = torch.cat([cr[1:], cr[-1:] + 1]) if int(cr[-1]) + 1 < C.shape[0] else torch.cat([cr[1:], cr[:1]])
        if case.epi == EPI_SWIGLU:
            gt, up = _pair(acc)
            if mutant == "swiglu_swap":
                gt, up = gt.clone(), up.clone()
                gt[:, -16:], up[:, -16:] = _pair(acc)[1][:, -16:], _pair(acc)[0][:, -16:]
            out = (_bf(_act32(_bf(gt), EPI_SILU)) * _bf(up)).to(BF16)
        else:
            o = acc
            b = g["bias"].float() if g["bias"] is not None else None
            if b is not None and mutant == "bias_chunk_prev" and N >= 16:
                b = b.clone()
                b[N - 8:] = b[N - 16:N - 8]
            if mutant == "bias_after_rounding" and b is not None:
                o = _bf(o) + b
            elif b is not None:
                o = o + b
            if case.epi in (EPI_GELU, EPI_SILU):
                o = _act32(o if mutant == "gelu_unrounded" else _bf(o), case.epi)
            if case.res:
                r = C[cr, :Nout].float()
                o = (o + r) if mutant == "merged_residual" else (_bf(o) + r)
            out = o.to(BF16)
        C[cr, :Nout] = out
        if mutant == "clamp_dup":                                     # the row past the group's last: written with the clamped (last) row
            last = int(cr[-1])
            if last + 1 < C.shape[0]:
                C[last + 1, :Nout] = out[-1]
    return C


def matmul32(case):
    """An honest fp32 torch.matmul with the rounding sequence (no schedule)."""
    C = case.C0.clone()
    for g in case.groups:
        acc = case.A[case.arows(g)].float() @ g["W"].float().t()
        cr = case.crows(g)
        if case.epi == EPI_SWIGLU:
            gt, up = _pair(acc)
            out = (_bf(_act32(_bf(gt), EPI_SILU)) * _bf(up)).to(BF16)
        else:
            o = acc + g["bias"].float() if g["bias"] is not None else acc
            if case.epi in (EPI_GELU, EPI_SILU):
                o = _act32(_bf(o), case.epi)
            if case.res:
                o = _bf(o) + C[cr, :case.Nout].float()
            out = o.to(BF16)
        C[cr, :case.Nout] = out
    return C


def passes(case, got, ref=None):
    try:
        assert_case(case, got, ref)
        return True
    except AssertionError:
        return False


def fp8_exact(M, N, K, seed=0):
    """The exact family for the fp8 GEMM: codes +-1 / 0, per-row scales 2^-3 .. 2^3 -> (codes A [M, K], sa [M], codes W [N, K], sw [N]) as fp32 and the
    bf16 operands A sa / W sw of the equivalent bf16 problem (exact: powers of two)."""
    p = fam_exact(M, N, K, seed=seed)
    g = _gen(16, seed, M, N)
    sa = 2.0 ** torch.randint(-3, 4, (M,), generator=g).float()
    sw = 2.0 ** torch.randint(-3, 4, (N,), generator=g).float()
    return p, sa, sw


# ------------------------------------------------------------------------------------------------------------
# running a Case through bagel_amd.ops (the caller passes the module: nothing here imports the GPU)
# ------------------------------------------------------------------------------------------------------------
def gemm_args(case, dev="cuda"):
    """Device operands of ``case`` for ops.gemm: (A, W0, keyword arguments)."""
    i32 = lambda x: None if x is None else torch.tensor(x, dtype=torch.int32, device=dev)  # noqa: E731
    g0 = case.groups[0]
    g1 = case.groups[1] if len(case.groups) > 1 else None
    kw = dict(bias0=None if g0["bias"] is None else g0["bias"].to(dev), a_rows0=i32(g0["a_rows"]), c_rows0=i32(g0["c_rows"]), M0=g0["M"], epilogue=case.epi)
    if g1 is not None:
        kw.update(W1=g1["W"].to(dev), bias1=None if g1["bias"] is None else g1["bias"].to(dev), a_rows1=i32(g1["a_rows"]), c_rows1=i32(g1["c_rows"]), M1=g1["M"])
    return case.A.to(dev), g0["W"].to(dev), kw


def run_gemm(ops, case, args, variant, **extra):
    """ops.gemm on a fresh copy of the case's C buffer (residual in place) -> the whole buffer on the host."""
    A, W, kw = args
    C = case.C0.to(A.device).clone()
    Cv = C[:, :case.Nout]
    ops.gemm(A, W, Cv, residual=Cv if case.res else None, variant=variant, **kw, **extra)
    return C.cpu()


def run_dense(fn, case, dev="cuda", A=None, **extra):
    """A dense single-group case through ops.gemm_skinny / gemv / gemv_mb (``fn``): M rows of padded buffers, residual in place."""
    g = case.groups[0]
    assert len(case.groups) == 1 and g["a_rows"] is None and g["c_rows"] is None
    C = case.C0.to(dev).clone()
    Cv = C[:, :case.Nout]
    fn((case.A if A is None else A).to(dev), g["W"].to(dev), Cv, bias=None if g["bias"] is None else g["bias"].to(dev), residual=Cv if case.res else None,
       epilogue=case.epi, M=g["M"], **extra)
    return C.cpu()
