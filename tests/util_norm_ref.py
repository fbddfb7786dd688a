"""Float64 reference, legal bit patterns, designed input families and an fp32 restatement (+ wrong variants) of the row norms and rotary
embeddings: norm.hip (rmsnorm, rmsnorm_fp8, layernorm, rope_table, qknorm_rope, rope2d) and decode_qkv_post_kernel of decode.hip.  Pure
torch on the CPU; tests/test_norm_ref_cpu.py validates it, tests/test_norm_designed_gpu.py applies it to the HIP kernels.

THE ROUNDING SEQUENCES (bfround / pack2bf / f2bf: fp32 -> bf16, round to nearest even; the build runs with -ffp-contract=off)

  rmsnorm        ss = sum x^2 (fp32, lane then wave order)            norm.hip `ss += a * a + b * b;` `ss = wave_sum(ss);`
                 inv = rsqrtf(ss / cols + eps)                        `const float inv = rsqrtf(ss / (float)cols + eps);`
                 y = bf16(bf16(x * inv) * w)                          `bfround(lo2f(v[i][e]) * inv) * lo2f(g[i][e])` -> `pack2bf(a, b)`
                 both the register form (cols <= 4096) and the streaming form spell these lines; w = w1 where expert[row] != 0
  rmsnorm_fp8    the same y, then y / s -> e4m3, s = max|y| / 448     `bfround(bfround(lo2f(v[e]) * inv) * lo2f(g[e]))`; checked against rmsnorm
                                                                      followed by the quantiser, as tests/test_fp8_gpu.py does
  layernorm      mean = (sum x) / cols;  c = x - mean (fp32)          `const float mean = wave_sum(s) / (float)cols;` `lo2f(v[e]) - mean`
                 inv = rsqrtf(sum c^2 / cols + eps)                   `const float inv = rsqrtf(wave_sum(ss) / (float)cols + eps);`
                 y = bf16(c * inv * w + b)     all fp32, one rounding `pack2bf((lo2f(v[e]) - mean) * inv * lo2f(g[e]) + lo2f(bb[e]), ..)`
  rope_table     ang = fl32(pos * inv_freq); bf16(cosf(ang)), bf16(sinf(ang))    `__fmul_rn((float)pos[r], inv_freq[c])` `f2bf(cosf(ang))`
  qknorm_rope    per head of HD elements (pad lanes [HD, DP) and the V heads are not touched), table column e mod HD/2, rot = -x[e + HD/2] in
                 the lower half and +x[e - HD/2] in the upper one
      norm       inv = rsqrtf(ss / HD + eps)                          `const float inv = rsqrtf(ss / (float)HD + eps);`
        und      n = bf16(w * bf16(x * inv))                          `nrm[e] = bfround(wf[e] * bfround(x[e] * inv));`
        gen      n = fl32(w * fl32(x * inv))                          `nrm[e] = __fmul_rn(wf[e], __fmul_rn(x[e], inv));`
        no norm  n = x                                                `nrm[e] = x[e];`
      rope und   out = bf16(bf16(n * cos) + bf16(rot * sin))          `out[e] = bfround(nrm[e] * cs[e]) + bfround(rot * sn[e]);` -> pack2bf
           gen   out = bf16(fl32(fl32(n * cos) + fl32(rot * sin)))    `out[e] = __fadd_rn(__fmul_rn(nrm[e], cs[e]), __fmul_rn(rot, sn[e]));`
  decode_qkv_post  the und lines of qknorm_rope word for word (decode.hip `nrm[e] = bfround(wf[e] * bfround(x[e] * inv));`, `out[e] =
                 bfround(nrm[e] * cs[e]) + bfround(rot * sn[e]);`); q in place, the K head and the raw V head (`is_v ? xr[e] : pack2bf(..)`)
                 to pool row block_table[b, j / 64] * 64 + j % 64 with j = kv_len[b], pad lanes of that row zeroed (`*(unsigned*)(dst + off
                 + 2 * e) = 0u;`)
  rope2d         per half (0: row tables, 1: column tables) of a head, j < HD / 4, tables indexed by pos_ids[row]:
                 o1 = bf16(bf16(x1 c[j]) + bf16(-x2 s[j])), o2 = bf16(bf16(x2 c[j + q4]) + bf16(x1 s[j + q4]))
                                                                      `bfround(x1 * bf2f(ct[j])) + bfround(-x2 * bf2f(st[j]))`

WHAT IS LEGAL
  No reduction -> ONE bit pattern.  rope2d, qknorm_rope(use_norm = 0) in both modes and decode_qkv_post(use_norm = 0): the product of two bf16
  values is exact in fp32, every bfround and the fp32 sum are IEEE operations, so ``emu_*`` (fp32 torch) gives the kernel's bits on every input.
  Row norms: the only freedom is inv.  inv64 = the float64 value from the bf16 inputs; the kernel's inv lies in inv64 (1 +- delta),
      delta(n) = ((n + 1) 2^-24) / 2 + rho
  (n + 1) 2^-24: the sum of n non-negative squares (each exact in fp32: 16 significant bits) in ANY order errs by at most (n - 1) 2^-24
  relative, the division and the eps sum add one each; the inverse square root halves a relative error; rho is rsqrtf's own.  bf16(fl32(x *
  inv)) is monotone in inv, so the first rounding is one of n1 in {bf16(x inv64 (1 - delta)), bf16(x inv64 (1 + delta))} (asserted: at most
  one bf16 step apart).  und: the legal results are bf16(w n1) (rmsnorm) and, for qknorm, bf16(bf16(n cos) + bf16(rot sin)) over the
  candidates of the element and of its partner.  gen: v = w x inv64 cos + rot sin in float64 and every fp32 result within
      B = (delta + 3 * 2^-24)(|w x inv cos| + |rot sin|)(1 + 2^-10) + 2^-24 |v|
  (three product roundings per term, the rounding of the sum), so the legal outputs are the bf16 values from bf16(v - B) to bf16(v + B).
  layernorm (n columns, e = 2^-24, A = mean |x|, c = x - mean64, var = mean c^2, inv = 1 / sqrt(var + eps), t = c inv w + b, all float64)
      e_mu  = (n + 1) e A                                    n - 1 additions in any order, each partial sum <= n A, + the division
              (pivot family: e |mean|                        its rows sum exactly in fp32 in any order, asserted; the division alone rounds)
      e_c,i = e_mu + e (|c_i| + e_mu)                        the carried mean + the rounding of the difference
      e_var = (2 e var + 2 e e_mu mean|c| + e_c,max^2)       sum c~^2 - sum c^2 = 2 sum c_i d_i + sum d_i^2 with d_i = -dmu + r_i; the dmu
              / (var + eps) + (n + 2) e                      part of the cross term vanishes (sum c_i = 0): that keeps the bound finite and tight
                                                             where |x| >> |x - mean|; (n + 2) e: squares, additions, division, eps sum
      e_inv = e_var / 2 + rho
      E_i   = |w_i| inv (e_c,i + |c_i| (e_inv + 2 e)) + e |t_i|        two products and the sum with the bias
      |got - t| <= u |t| + (1 + u) E,  u = 2^-8;   AND got lies between bf16(t - E) and bf16(t + E) (the one output rounding; this is what
      rejects a bias added after a rounding)
  rope_table: the angle is the same fp32 number on both sides; the legal values are the bf16 values from bf16(c64 - a) to bf16(c64 + a).
  rho and a: the ROCm documentation states no accuracy for the device rsqrtf / cosf / sinf on gfx950 (nor for v_rsq_f32 itself), so tools/libm_accuracy_probe.hip measured the device functions against float64 (profiles/libm_accuracy_gfx950.txt):
      rsqrtf  2^22 arguments in [2^-30, 2^20]: worst relative error 1.565 * 2^-24         -> RHO    = 3.13 * 2^-24 (twice the observed)
      cosf / sinf  2^22 + 2^22 arguments in [0, 32768] and every table angle of positions < 32768 at head dims 32, 72, 128:
              worst absolute error 1.170 * 2^-24                                            -> A_TRIG = 2.34 * 2^-24
              worst error in units of the result's fp32 spacing 1.574 (relative <= 1.574 * 2^-23)  -> R_TRIG = 3.15 * 2^-23
      Both held at every probed argument, so a = min(A_TRIG, R_TRIG |c64|): the absolute figure alone would let sin of a small angle (1e-6 at
      position 1) be anything within 1.4e-7.
  A legal set with more than one member proves little, so ``Legal.ambiguous`` is reported and bounded (<= 1/8 per real-valued case, 0 on the
  exact families) by the tests.

FAMILIES (seeded; each asserts its own precondition)
  exact      x = a m: per 8 elements a permutation with random signs of {5,2,1,1,1,0,0,0}, {3,3,3,2,1,0,0,0}, {4,2,2,2,2,0,0,0} or {4,4,0,..}
             (squares sum to 32), a = 2^k per row with 4 a^2 + eps == 4 a^2 in fp32, w multiples of 1/8 in [1/2, 2): mean square 4 a^2 in any
             order, x inv = m / 2 (1 +- few 2^-24) -> bf16 m / 2, w m / 2 has <= 7 bits: one pattern.  qknorm: tables with one of cos / sin zero
             per entry and the other +-1 / +-2, so the gen chain's fp32 dust cannot meet a rounding boundary or a cancellation.
  tables     cos / sin are inputs: 5-bit dyadic values that encode (row, column) (four different ones for rope2d, indexed through a pos_ids
             that is a permutation with repeats); x small integers.
  castpoint  x = 3 randn, w = 1 + 0.1 randn, oracle-style tables at positions up to 32000.
  tiny       rows at scale 2^-10, 2^-11, 2^-12 mixed with rows at 2^6: eps decides the small rows.
  pivot      layernorm: all entries P = 256 except 1/16 at 258 and 1/16 at 254 (mean exactly P, centred values {0, +-2}, variance 1/2); the second
             magnitude P = 4080 with 1/16 at 4096 and one entry fewer at 4064.  Row sums are exact in fp32 in any order.
  benign     layernorm: x = 3 randn; beyond 1152 columns on the grid 1/8 (tiny: scale / 8), so that the row sum is exact in any order: the any-order
             bound of the mean, (n + 1) 2^-24 mean|x|, would otherwise leave a quarter of the elements with two legal patterns at 4104 columns.
  Buffers are larger than the problem: x columns past ``cols`` hold NaN, everything the kernel must not write holds SENTINEL.
"""
import math

import torch

from tests.util_gemm_ref import bf16_step, bits

BF16 = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
E24 = 2.0 ** -24
U = 2.0 ** -8
RHO = 3.13 * E24            # twice the worst relative error of rsqrtf observed by tools/libm_accuracy_probe.hip (1.565 * 2^-24)
A_TRIG = 2.34 * E24         # twice the worst absolute error of cosf / sinf observed there (1.170 * 2^-24)
R_TRIG = 3.15 * 2.0 ** -23  # twice their worst error in units of the result's own fp32 spacing (1.574 ulp): what holds sin of a small angle
SENTINEL = -1232.0          # exact in bf16; no family produces it
KV_PAGE = 64


def delta(n):
    return (n + 1) * E24 / 2 + RHO


def rne(x64):
    """float64 -> fp32 -> bf16, the kernels' two roundings."""
    return x64.to(F32).to(BF16)


def _bf(x):
    return x.to(BF16).to(F32)


def _gen(*seed):
    s = 0
    for x in seed:
        s = (s * 1000003 + int(x) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _key(x):
    """bf16 -> int32, ordered like the values (-0 == +0)."""
    b = bits(x).to(torch.int32) & 0xFFFF
    return torch.where(b >= 0x8000, -(b & 0x7FFF), b)


class Legal:
    """The legal results of a region: a list of candidate tensors (membership) or an interval [lo, hi] of bf16 values."""

    def __init__(self, cands=None, lo=None, hi=None):
        self.cands, self.lo, self.hi = cands, lo, hi
        if cands is None:
            klo, khi = _key(lo), _key(hi)
            self.klo, self.khi = torch.minimum(klo, khi), torch.maximum(klo, khi)

    def ok(self, got):
        if self.cands is None:
            k = _key(got)
            return (k >= self.klo) & (k <= self.khi) & torch.isfinite(got.float())
        r = torch.zeros(got.shape, dtype=torch.bool)
        for c in self.cands:
            r |= _key(c) == _key(got)
        return r & torch.isfinite(got.float())

    def ambiguous(self):
        if self.cands is None:
            return self.klo != self.khi
        r = torch.zeros(self.cands[0].shape, dtype=torch.bool)
        for c in self.cands[1:]:
            r |= _key(c) != _key(self.cands[0])
        return r

    def share(self):
        a = self.ambiguous()
        return float(a.float().mean()) if a.numel() else 0.0


def check(name, got, buf0, region, legal, what=""):
    """``got``: the whole buffer after the call; ``region``: bool mask of what must be written (row-major order = the order of ``legal``).
    Everything else must equal ``buf0`` bit for bit.  -> the ambiguous share of the region."""
    assert got.shape == buf0.shape and got.dtype == buf0.dtype, (name, got.shape, buf0.shape)
    bad = (bits(got) != bits(buf0)) & ~region
    if bool(bad.any()):
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what} {name}: element {i} outside the result was overwritten with {got[tuple(i)].item()} ({int(bad.sum())} elements)")
    g = got[region]
    ok = legal.ok(g.view(legal.ambiguous().shape))
    if not bool(ok.all()):
        i = (~ok).nonzero()[0].tolist()
        flat = (~ok).flatten().nonzero()[0].item()
        where = region.nonzero()[flat].tolist()
        c = [x[tuple(i)].item() for x in legal.cands] if legal.cands is not None else [legal.lo[tuple(i)].item(), legal.hi[tuple(i)].item()]
        raise AssertionError(f"{what} {name}: {int((~ok).sum())} of {ok.numel()} elements are no legal result; first at buffer index {where}: "
                             f"got {g.flatten()[flat].item()!r}, legal {'set' if legal.cands is not None else 'interval'} {c}")
    return legal.share()


def passes(*a, **k):
    try:
        check(*a, **k)
        return True
    except AssertionError:
        return False


# ------------------------------------------------------------------------------------------------------------
# families of rows
# ------------------------------------------------------------------------------------------------------------
PATTERNS = ((5, 2, 1, 1, 1, 0, 0, 0), (3, 3, 3, 2, 1, 0, 0, 0), (4, 2, 2, 2, 2, 0, 0, 0), (4, 4, 0, 0, 0, 0, 0, 0))


def fam_exact_rows(rows, cols, seed=0, eps=1e-6):
    """-> x [rows, cols] bf16 and the row scales a [rows]."""
    g = _gen(21, seed, rows, cols)
    nb = rows * (cols // 8)
    pat = torch.tensor(PATTERNS, dtype=F32)[torch.randint(0, 4, (nb,), generator=g)]
    pat = torch.gather(pat, 1, torch.rand((nb, 8), generator=g).argsort(1))
    pat = pat * (torch.randint(0, 2, (nb, 8), generator=g) * 2 - 1)
    a = 2.0 ** (2 + torch.arange(rows) % 4).float()
    x = pat.view(rows, cols) * a[:, None]
    assert bool((pat.pow(2).sum(1) == 32).all())
    m4 = 4 * a * a
    assert bool(((m4 + torch.tensor(eps, dtype=F32)) == m4).all()), "exact: 4 a^2 + eps must round back to 4 a^2"
    assert bool((x.to(BF16).float() == x).all())
    return x.to(BF16), a


def exact_weight(n, seed):
    return (torch.randint(4, 16, (n,), generator=_gen(22, seed, n)).float() / 8).to(BF16)


def real_weight(n, seed):
    return (1 + 0.1 * torch.randn(n, generator=_gen(23, seed, n))).to(BF16)


def fam_real_rows(family, rows, cols, seed=0):
    g = _gen(24, seed, rows, cols)
    x = torch.randn(rows, cols, generator=g)
    if family == "tiny":
        sc = torch.tensor([2.0 ** -10, 2.0 ** 6, 2.0 ** -11, 2.0 ** -12])[torch.arange(rows) % 4]
        x = x * sc[:, None]
        x = x.to(BF16)
        ms = x.double().pow(2).mean(1)
        assert rows < 1 or float(ms.min()) < 4e-6, "tiny: eps must matter on the small rows"
        return x
    assert family in ("castpoint", "benign")
    return (x * 3).to(BF16)


# ------------------------------------------------------------------------------------------------------------
# rmsnorm
# ------------------------------------------------------------------------------------------------------------
class RowCase:
    """x [rows, ldx] (columns past cols: NaN), w0 / w1 / expert, bias (layernorm), y0 [rows + 2, ldy] full of SENTINEL."""

    def __init__(self, name, x, w0, w1, expert, cols, ldy, eps, bias=None, exact=False):
        self.name, self.w0, self.w1, self.expert, self.cols, self.eps, self.bias, self.exact = name, w0, w1, expert, cols, eps, bias, exact
        self.rows = x.shape[0]
        self.x = x
        self.y0 = torch.full((self.rows + 2, ldy), SENTINEL, dtype=BF16)
        self.region = torch.zeros(self.y0.shape, dtype=torch.bool)
        self.region[:self.rows, :cols] = True

    def xv(self):
        return self.x[:, :self.cols]

    def weight(self, swap=False):
        w = self.w0.float()[None].expand(self.rows, -1)
        if self.expert is not None:
            e = self.expert.bool() ^ swap
            w = torch.where(e[:, None], self.w1.float()[None], self.w0.float()[None])
        return w


def _pad_x(x, ldx):
    buf = torch.full((x.shape[0], ldx), float("nan"), dtype=BF16)
    buf[:, :x.shape[1]] = x
    return buf


def rms_case(family, rows, cols, ldx=None, ldy=None, routed=None, seed=0, eps=1e-6):
    """routed: None (no expert list), "mixed", "zeros", "ones"."""
    ldx, ldy = ldx or cols + 8, ldy or cols + 16
    if family == "exact":
        x, _ = fam_exact_rows(rows, cols, seed, eps)
        w0, w1 = exact_weight(cols, seed), exact_weight(cols, seed + 1)
    else:
        x = fam_real_rows(family, rows, cols, seed)
        w0, w1 = real_weight(cols, seed), real_weight(cols, seed + 1)
    ex = None
    if routed is not None:
        ex = {"mixed": (torch.arange(rows) % 3 == 1), "zeros": torch.zeros(rows, dtype=torch.bool), "ones": torch.ones(rows, dtype=torch.bool)}[routed].to(torch.int32)
        assert routed != "mixed" or cols < 16 or not torch.equal(w0, w1)
    return RowCase(f"rmsnorm {family} {rows}x{cols} ld {ldx}/{ldy} {routed}", _pad_x(x, ldx), w0, w1 if routed else None, ex, cols, ldy, eps, exact=family == "exact")


def _inv64(x64, n, eps):
    return 1.0 / torch.sqrt(x64.pow(2).sum(-1, keepdim=True) / n + float(torch.tensor(eps, dtype=F32)))


def _n1_candidates(x64, inv64, n):
    d = delta(n)
    lo, hi = rne(x64 * inv64 * (1 - d)), rne(x64 * inv64 * (1 + d))
    assert bool(((_key(lo) - _key(hi)).abs() <= 1).all()), "the first rounding has more than two candidates"
    return lo, hi


def rms_legal(case):
    x = case.xv().double()
    lo, hi = _n1_candidates(x, _inv64(x, case.cols, case.eps), case.cols)
    w = case.weight()
    L = Legal(cands=[(lo.float() * w).to(BF16), (hi.float() * w).to(BF16)])
    assert not case.exact or L.share() == 0.0, "exact family: more than one legal pattern"
    return L


RMS_MUTANTS = ("merged_rounding", "eps_dropped", "eps_after_rsqrt", "divisor_ld", "wrong_expert", "tail_chunk_dropped")


def emu_rmsnorm(case, mutant=None):
    """-> the y buffer an honest (mutant = None) fp32 kernel leaves."""
    y = case.y0.clone()
    if case.rows == 0:
        return y
    x = case.xv().float()
    sq = x * x
    if mutant == "tail_chunk_dropped":
        nch = case.cols // 8
        sq = sq[:, :8 * (nch - nch % 64)]
    ms = sq.sum(-1, keepdim=True) / float(case.x.shape[1] if mutant == "divisor_ld" else case.cols)
    eps = torch.tensor(case.eps, dtype=F32)
    if mutant == "eps_dropped":
        inv = torch.rsqrt(ms)
    elif mutant == "eps_after_rsqrt":
        inv = torch.rsqrt(ms) + eps
    else:
        inv = torch.rsqrt(ms + eps)
    w = case.weight(swap=mutant == "wrong_expert")
    out = (x * inv * w) if mutant == "merged_rounding" else (_bf(x * inv) * w)
    y[:case.rows, :case.cols] = out.to(BF16)
    return y


def run_rmsnorm(ops, case, dev="cuda"):
    y = case.y0.to(dev).clone()
    d = lambda t: None if t is None else t.to(dev)  # noqa: E731
    ops.rmsnorm(case.x.to(dev)[:, :case.cols], d(case.w0), y[:case.rows, :case.cols], case.eps, w1=d(case.w1), expert=d(case.expert))
    return y.cpu()


# ------------------------------------------------------------------------------------------------------------
# layernorm
# ------------------------------------------------------------------------------------------------------------
def fam_pivot(rows, cols, seed=0):
    """Even rows: P = 256 with k = cols / 16 entries (at least one) at 258 and as many at 254: mean exactly 256, centred values {0, +-2}.  Odd rows, the
    second magnitude: P = 4080 = 255 * 16 with k entries at 4096 and k - 1 at 4064, so the sum of squares is an odd multiple of 16^2 (inexact in fp32
    past 2^24) and the mean is no fp32 number times a power of two."""
    g = _gen(25, seed, rows, cols)
    k = max(1, cols // 16)
    x = torch.empty(rows, cols)
    for r in range(rows):
        P, d, km = (256.0, 2.0, k) if r % 2 == 0 else (4080.0, 16.0, k - 1)
        p = torch.rand(cols, generator=g).argsort()
        x[r] = P
        x[r, p[:k]] = P + d
        x[r, p[k:k + km]] = P - d
        assert r % 2 or float(x[r].double().mean()) == P
        assert bool((x[r] % d == 0).all()) and cols * (P + d) <= 2 ** 24 * d, "pivot: the sum of a row must be exact in fp32 in any order"
    assert bool((x.to(BF16).float() == x).all())
    return x.to(BF16)


def ln_case(family, rows, cols, ldx=None, ldy=None, seed=0, eps=1e-6):
    ldx, ldy = ldx or cols + 8, ldy or cols + 16
    x = fam_pivot(rows, cols, seed) if family == "pivot" else fam_real_rows(family, rows, cols, seed)
    grid = family != "pivot" and cols > 1152
    if grid:
        sc = 2.0 ** torch.floor(torch.log2(x.float().pow(2).mean(1, keepdim=True).sqrt().clamp_min(1e-30))) / 8 if rows else torch.ones(0, 1)
        x = (torch.round(x.float() / sc) * sc).to(BF16)
        assert bool(((x.float() / sc).abs() <= 255).all()) and bool((x.float() / sc == torch.round(x.float() / sc)).all()) and cols * 255 <= 2 ** 24
    w = real_weight(cols, seed)
    b = (0.1 * torch.randn(cols, generator=_gen(26, seed, cols))).to(BF16)
    if family == "pivot":                                             # most centred values are zero: the result there is the bias alone
        b = ((0.5 + torch.rand(cols, generator=_gen(26, seed, cols))) * (torch.randint(0, 2, (cols,), generator=_gen(26, seed, cols + 1)) * 2 - 1)).to(BF16)
    if family == "tiny":
        b = (b.float() * 2.0 ** -3).to(BF16)
    case = RowCase(f"layernorm {family} {rows}x{cols} ld {ldx}/{ldy}", _pad_x(x, ldx), w, None, None, cols, ldy, eps, bias=b)
    case.exact_sum = family == "pivot" or grid
    return case


def ln_reference(case):
    """-> t, E, bound (float64 [rows, cols]) and the Legal interval."""
    n = case.cols
    x = case.xv().double()
    eps = float(torch.tensor(case.eps, dtype=F32))
    mu = x.mean(-1, keepdim=True)
    c = x - mu
    var = c.pow(2).mean(-1, keepdim=True)
    inv = 1.0 / torch.sqrt(var + eps)
    w, b = case.w0.double()[None], case.bias.double()[None]
    t = c * inv * w + b
    e_mu = (n + 1) * E24 * x.abs().mean(-1, keepdim=True)
    if getattr(case, "exact_sum", False):                             # every partial sum is exact (fam_pivot asserts it): the division alone rounds
        e_mu = E24 * mu.abs()
    e_c = e_mu + E24 * (c.abs() + e_mu)
    e_var = (2 * E24 * var + 2 * E24 * e_mu * c.abs().mean(-1, keepdim=True) + e_c.max(-1, keepdim=True).values ** 2) / (var + eps) + (n + 2) * E24
    e_inv = e_var / 2 + RHO
    E = w.abs() * inv * (e_c + c.abs() * (e_inv + 2 * E24)) + E24 * t.abs()
    bound = U * t.abs() + (1 + U) * E
    return dict(t=t, E=E, bound=bound, legal=Legal(lo=rne(t - E), hi=rne(t + E)))


def ln_ratio(case, got, ref):
    """Worst |got - t| / bound over the result."""
    g = got[:case.rows, :case.cols].double()
    q = (g - ref["t"]).abs() / ref["bound"].clamp_min(1e-300)
    q = torch.where(torch.isfinite(g), q, torch.full_like(q, float("inf")))
    return float(q.max()) if q.numel() else 0.0


LN_MUTANTS = ("one_pass_variance", "unbiased_variance", "bias_after_rounding", "eps_dropped")


def emu_layernorm(case, mutant=None):
    y = case.y0.clone()
    if case.rows == 0:
        return y
    n = case.cols
    x = case.xv().float()
    mean = x.sum(-1, keepdim=True) / float(n)
    c = x - mean
    if mutant == "one_pass_variance":
        var = (x * x).sum(-1, keepdim=True) / float(n) - mean * mean
    else:
        var = (c * c).sum(-1, keepdim=True) / float(n - 1 if mutant == "unbiased_variance" else n)
    inv = torch.rsqrt(var if mutant == "eps_dropped" else var + torch.tensor(case.eps, dtype=F32))
    o = c * inv * case.w0.float()[None]
    o = (_bf(o) + case.bias.float()[None]) if mutant == "bias_after_rounding" else (o + case.bias.float()[None])
    y[:case.rows, :n] = o.to(BF16)
    return y


def run_layernorm(ops, case, dev="cuda"):
    y = case.y0.to(dev).clone()
    ops.layernorm(case.x.to(dev)[:, :case.cols], case.w0.to(dev), case.bias.to(dev), y[:case.rows, :case.cols], case.eps)
    return y.cpu()


# ------------------------------------------------------------------------------------------------------------
# rope_table
# ------------------------------------------------------------------------------------------------------------
def inv_freq(hd, theta=1e6):
    return 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.int64).float() / hd))


def rope_table_legal(pos, inv):
    """-> (Legal of cos, Legal of sin), [rows, half]."""
    ang = (pos.to(F32)[:, None] * inv.to(F32)[None, :]).double()      # the fp32 product, exactly
    c, s = torch.cos(ang), torch.sin(ang)
    ac, as_ = (R_TRIG * c.abs()).clamp_max(A_TRIG), (R_TRIG * s.abs()).clamp_max(A_TRIG)
    return Legal(lo=rne(c - ac), hi=rne(c + ac)), Legal(lo=rne(s - as_), hi=rne(s + as_))


ROPE_TABLE_MUTANTS = ("angle_in_float64",)


def emu_rope_table(pos, inv, mutant=None):
    if mutant == "angle_in_float64":
        ang = pos.double()[:, None] * inv.double()[None, :]
        return torch.cos(ang).to(F32).to(BF16), torch.sin(ang).to(F32).to(BF16)
    ang = pos.to(F32)[:, None] * inv.to(F32)[None, :]
    return torch.cos(ang).to(BF16), torch.sin(ang).to(BF16)


def real_tables(pos, hd, theta=1e6):
    c, s = emu_rope_table(pos, inv_freq(hd, theta))
    return c.contiguous(), s.contiguous()


# ------------------------------------------------------------------------------------------------------------
# qknorm_rope and decode_qkv_post
# ------------------------------------------------------------------------------------------------------------
def designed_tables(nrow, half, k=0):
    """5-bit dyadic values that encode (row, column); ``k`` selects one of several different table pairs."""
    r, c = torch.arange(nrow)[:, None], torch.arange(half)[None, :]
    cos = (((r * (7 + 2 * k) + c * 3 + k) % 31) - 15).float() / 16
    sin = (((r * 5 + c * (11 + 2 * k) + 3 * k) % 29) - 14).float() / 8
    return cos.to(BF16).contiguous(), sin.to(BF16).contiguous()


def axis_tables(nrow, half, seed=0):
    """One of cos / sin zero per entry, the other +-1 or +-2."""
    g = _gen(27, seed, nrow, half)
    v = (torch.randint(1, 3, (nrow, half), generator=g) * (torch.randint(0, 2, (nrow, half), generator=g) * 2 - 1)).float()
    pick = torch.randint(0, 2, (nrow, half), generator=g).bool()
    return torch.where(pick, v, torch.zeros(())).to(BF16).contiguous(), torch.where(pick, torch.zeros(()), v).to(BF16).contiguous()


class QKCase:
    """qkv0 [rows + 1, ld]: q and k heads hold values in [0, hd) and SENTINEL in the pad lanes (qknorm_rope) or zeros (decode: ``pools``), V heads
    random values, columns past the heads and the last row SENTINEL.  Tables [rows, hd / 2]; weights q0 k0 q1 k1 [hd]; expert [rows] | None."""

    def __init__(self, name, x, v, nq, nkv, hd, dp, ld, cos, sin, w, expert, gen, use_norm, eps, exact, pad_value=SENTINEL):
        self.name, self.nq, self.nkv, self.hd, self.dp, self.cos, self.sin, self.w, self.expert = name, nq, nkv, hd, dp, cos, sin, w, expert
        self.gen, self.use_norm, self.eps, self.exact = gen, use_norm, eps, exact
        self.rows = rows = x.shape[0]
        H = nq + nkv
        buf = torch.full((rows + 1, ld), SENTINEL, dtype=BF16)
        heads = torch.full((rows, H, dp), pad_value, dtype=BF16)
        heads[:, :, :hd] = x
        vh = torch.full((rows, nkv, dp), pad_value, dtype=BF16)
        vh[:, :, :hd] = v
        buf[:rows, :(H + nkv) * dp] = torch.cat([heads.reshape(rows, H * dp), vh.reshape(rows, nkv * dp)], 1)
        self.qkv0 = buf
        reg = torch.zeros(rows, H + nkv, dp, dtype=torch.bool)
        reg[:, :H, :hd] = True
        self.region = torch.zeros(buf.shape, dtype=torch.bool)
        self.region[:rows, :(H + nkv) * dp] = reg.reshape(rows, (H + nkv) * dp)

    def heads(self, buf=None):
        """[rows, nq + nkv, hd] view of the q and k values."""
        buf = self.qkv0 if buf is None else buf
        H = self.nq + self.nkv
        return buf[:self.rows, :H * self.dp].reshape(self.rows, H, self.dp)[:, :, :self.hd]

    def vheads(self):
        H = self.nq + self.nkv
        return self.qkv0[:self.rows, H * self.dp:(H + self.nkv) * self.dp].reshape(self.rows, self.nkv, self.dp)

    def weights(self, ignore_expert=False, k_uses_q=False):
        """[rows, nq + nkv, hd] fp32."""
        rows, nq, nkv, hd = self.rows, self.nq, self.nkv, self.hd
        ex = self.expert.bool() if (self.expert is not None and not ignore_expert) else torch.zeros(rows, dtype=torch.bool)
        q0, k0, q1, k1 = [None if t is None else t.float() for t in self.w]
        wq = torch.where(ex[:, None], q1[None], q0[None]) if q1 is not None else q0[None].expand(rows, -1)
        wk = torch.where(ex[:, None], k1[None], k0[None]) if k1 is not None else k0[None].expand(rows, -1)
        if k_uses_q:
            wk = wq
        return torch.cat([wq[:, None, :].expand(rows, nq, hd), wk[:, None, :].expand(rows, nkv, hd)], 1)


def qk_case(family, rows, nq, nkv, hd, dp, gen, use_norm, routed=None, seed=0, eps=1e-6, pad_value=SENTINEL, extra_ld=24):
    H = nq + nkv
    g = _gen(28, seed, rows, H, hd)
    exact = False
    if family == "exact":
        x, _ = fam_exact_rows(rows * H, hd, seed, eps)
        x = x.view(rows, H, hd)
        cos, sin = axis_tables(rows, hd // 2, seed)
        w = [exact_weight(hd, seed + i) for i in range(4)]
        exact = True
    elif family == "tables":
        x = torch.randint(-127, 128, (rows, H, hd), generator=g).float().to(BF16)
        cos, sin = designed_tables(rows, hd // 2)
        w = [exact_weight(hd, seed + i) for i in range(4)]
    else:
        x = fam_real_rows(family, rows * H, hd, seed).view(rows, H, hd)
        pos = torch.randint(0, 32001, (rows,), generator=g)
        if rows:
            pos[0], pos[-1] = 32000, 0
        cos, sin = real_tables(pos, hd)
        w = [real_weight(hd, seed + i) for i in range(4)]
    v = torch.randn(rows, nkv, hd, generator=g).to(BF16)
    ex = None
    if routed is not None:
        ex = {"mixed": (torch.arange(rows) % 4 != 0), "zeros": torch.zeros(rows, dtype=torch.bool), "ones": torch.ones(rows, dtype=torch.bool)}[routed].to(torch.int32)
    else:
        w[2] = w[3] = None
    ld = (H + nkv) * dp + extra_ld
    return QKCase(f"qknorm {family} rows {rows} heads {nq}+{nkv} hd {hd}/{dp} gen {gen} norm {use_norm} {routed}", x, v, nq, nkv, hd, dp, ld, cos, sin, w, ex,
                  gen, use_norm, eps, exact or not use_norm, pad_value=pad_value)


def _rot(n):
    h2 = n.shape[-1] // 2
    return torch.cat([-n[..., h2:], n[..., :h2]], -1)


def _tab(case, t, dtype):
    """[rows, hd / 2] table -> [rows, 1, hd] (column e mod hd / 2)."""
    return torch.cat([t, t], -1).to(dtype)[:, None, :]


def qk_legal(case):
    """Legal results of the q and k heads, [rows, nq + nkv, hd]."""
    hd = case.hd
    x = case.heads()
    if not case.use_norm:
        return Legal(cands=[_qk_chain(case, x.float(), None, None, case.gen)])
    x64 = x.double()
    inv = _inv64(x64, hd, case.eps)
    w = case.weights()
    c32, s32 = _tab(case, case.cos, F32), _tab(case, case.sin, F32)
    if not case.gen:
        lo, hi = _n1_candidates(x64, inv, hd)
        n = [(w * lo.float()).to(BF16).float(), (w * hi.float()).to(BF16).float()]
        cands = [(_bf(a * c32) + _bf(_rot(b) * s32)).to(BF16) for a in n for b in n]
        L = Legal(cands=cands)
    else:
        p = w.double() * x64 * inv
        a, b = p * c32.double(), _rot(p) * s32.double()
        v = a + b
        B = (delta(hd) + 3 * E24) * (a.abs() + b.abs()) * (1 + 2.0 ** -10) + E24 * v.abs()
        L = Legal(lo=rne(v - B), hi=rne(v + B))
    assert not case.exact or L.share() == 0.0, "exact family: more than one legal pattern"
    return L


def _qk_chain(case, x, w, inv, gen, rot_sign=1.0, cos=None, sin=None):
    """The fp32 restatement of one mode on [rows, heads, hd] fp32 values (w / inv None: no norm) -> bf16."""
    c32 = _tab(case, case.cos, F32) if cos is None else cos
    s32 = _tab(case, case.sin, F32) if sin is None else sin
    if w is None:
        n = x
    elif gen:
        n = w * (x * inv)
    else:
        n = _bf(w * _bf(x * inv))
    rot = _rot(n) * rot_sign
    out = (n * c32 + rot * s32) if gen else (_bf(n * c32) + _bf(rot * s32))
    return out.to(BF16)


QK_MUTANTS = ("und_in_gen", "gen_in_und", "divisor_dp", "rotate_sign", "cos_not_wrapped", "table_row_shift", "k_uses_q_weight", "expert_ignored",
              "v_written", "pad_written")


def _emu_heads(case, x, mutant, heads_w=None):
    """x [rows, heads, hd] fp32 -> bf16 results of the q / k chain with the case's mode."""
    hd = case.hd
    gen = case.gen
    if mutant == "und_in_gen" and gen:
        gen = 0
    if mutant == "gen_in_und" and not gen:
        gen = 1
    cos, sin = case.cos, case.sin
    if mutant == "table_row_shift":
        cos, sin = torch.roll(cos, -1, 0), torch.roll(sin, -1, 0)
    c32, s32 = _tab(case, cos, F32), _tab(case, sin, F32)
    if mutant == "cos_not_wrapped":               # element e reads flat table index row * hd / 2 + e: the upper half runs into the next row
        fc, fs = torch.cat([cos.flatten(), cos.flatten()[:hd]]).float(), torch.cat([sin.flatten(), sin.flatten()[:hd]]).float()
        idx = torch.arange(case.rows)[:, None] * (hd // 2) + torch.arange(hd)[None, :]
        c32, s32 = fc[idx][:, None, :], fs[idx][:, None, :]
    w = inv = None
    if case.use_norm:
        w = heads_w if heads_w is not None else case.weights(ignore_expert=mutant == "expert_ignored", k_uses_q=mutant == "k_uses_q_weight")
        inv = torch.rsqrt((x * x).sum(-1, keepdim=True) / float(case.dp if mutant == "divisor_dp" else hd) + torch.tensor(case.eps, dtype=F32))
    return _qk_chain(case, x, w, inv, gen, rot_sign=-1.0 if mutant == "rotate_sign" else 1.0, cos=c32, sin=s32)


def emu_qknorm(case, mutant=None):
    """-> the qkv buffer an honest (mutant = None) fp32 kernel leaves."""
    buf = case.qkv0.clone()
    rows, H, nkv, hd, dp = case.rows, case.nq + case.nkv, case.nkv, case.hd, case.dp
    if rows == 0:
        return buf
    out = _emu_heads(case, case.heads().float(), mutant)
    hv = buf[:rows, :(H + nkv) * dp].reshape(rows, H + nkv, dp).clone()
    hv[:, :H, :hd] = out
    if mutant == "pad_written" and dp > hd:
        hv[:, :H, hd:] = 0
    if mutant == "v_written":
        sub = QKCase("v", case.vheads()[:, :, :hd], case.vheads()[:, :, :hd], 0, nkv, hd, dp, 2 * nkv * dp, case.cos, case.sin, case.w, case.expert,
                     case.gen, case.use_norm, case.eps, False)
        hv[:, H:, :hd] = _emu_heads(sub, sub.heads().float(), None)
    buf[:rows, :(H + nkv) * dp] = hv.reshape(rows, -1)
    return buf


def run_qknorm(ops, case, dev="cuda"):
    buf = case.qkv0.to(dev).clone()
    d = lambda t: None if t is None else t.to(dev)  # noqa: E731
    w = [d(t) for t in case.w]
    if not case.use_norm:
        w = [None] * 4
    ops.qknorm_rope(buf[:case.rows], d(case.cos), d(case.sin), w[0], w[1], w[2], w[3], d(case.expert), case.nq, case.nkv, case.hd, case.dp,
                    case.eps, case.gen, case.use_norm)
    return buf.cpu()


class DecodeCase:
    """A QKCase (und, unrouted, rows = batch, pad lanes 3.0) + paged pools full of SENTINEL: block_table [B, 2] on scattered pages, kv_len."""

    def __init__(self, family, nq, nkv, hd, dp, use_norm, kv_len=(0, 63, 64, 127), npages=11, seed=0):
        B = len(kv_len)
        self.qk = qk_case(family, B, nq, nkv, hd, dp, 0, use_norm, seed=seed, pad_value=3.0)   # pads the kernel must not copy: the page rows get zeros
        self.name = "decode_qkv_post " + self.qk.name
        self.kv_len = torch.tensor(kv_len, dtype=torch.int32)
        perm = torch.rand(npages, generator=_gen(29, seed, npages)).argsort()[:2 * B]
        assert 2 * B <= npages and len(set(perm.tolist())) == 2 * B
        self.block_table = perm.view(B, 2).to(torch.int32).contiguous()
        assert not torch.equal(self.block_table.flatten().sort().values, self.block_table.flatten()), "pages must be scattered"
        self.ldp = nkv * dp + 8
        self.pool0 = torch.full((npages * KV_PAGE + 1, self.ldp), SENTINEL, dtype=BF16)
        self.prow = (self.block_table[torch.arange(B), (self.kv_len // KV_PAGE).long()].long() * KV_PAGE + (self.kv_len % KV_PAGE).long())
        self.pool_region = torch.zeros(self.pool0.shape, dtype=torch.bool)
        self.pool_region[self.prow, :nkv * dp] = True
        q = self.qk
        self.q_region = q.region.clone()
        self.q_region[:, q.nq * dp:] = False


DECODE_MUTANTS = ("pad_not_zeroed", "slot_off_by_one", "page_boundary", "head_tail_dropped", "v_roped")


def emu_decode(dc, mutant=None):
    """-> (qkv buffer, K pool, V pool) after an honest decode_qkv_post."""
    q = dc.qk
    B, nq, nkv, hd, dp = q.rows, q.nq, q.nkv, q.hd, q.dp
    out = _emu_heads(q, q.heads().float(), None)                  # [B, nq + nkv, hd]
    buf = q.qkv0.clone()
    hv = buf[:B, :nq * dp].reshape(B, nq, dp).clone()
    hv[:, :, :hd] = out[:, :nq]
    if mutant == "head_tail_dropped" and (nq + 2 * nkv) % 16:   # the last, partial block of 16 heads never runs
        done = (nq + 2 * nkv) // 16 * 16
        hv[:, done:nq] = buf[:B, :nq * dp].reshape(B, nq, dp)[:, done:nq]
    buf[:B, :nq * dp] = hv.reshape(B, -1)
    kp, vp = dc.pool0.clone(), dc.pool0.clone()
    krow = torch.full((B, nkv, dp), SENTINEL if mutant == "pad_not_zeroed" else 0.0, dtype=BF16)
    vrow = krow.clone()
    krow[:, :, :hd] = out[:, nq:]
    vrow[:, :, :hd] = q.vheads()[:, :, :hd]
    if mutant == "v_roped":
        vrow[:, :, :hd] = _emu_heads(q, q.vheads()[:, :, :hd].float(), None, heads_w=None if not q.use_norm else q.weights()[:, nq:])
    prow = dc.prow
    if mutant == "slot_off_by_one":
        prow = prow + 1
    if mutant == "page_boundary":                                  # the page of slot j taken as j / 64 rounded up
        j = dc.kv_len.long()
        prow = dc.block_table[torch.arange(B), ((j + KV_PAGE - 1) // KV_PAGE).clamp(max=1)].long() * KV_PAGE + j % KV_PAGE
    if mutant == "head_tail_dropped" and (nq + 2 * nkv) % 16:
        return buf, kp, vp
    kp[prow, :nkv * dp], vp[prow, :nkv * dp] = krow.reshape(B, -1), vrow.reshape(B, -1)
    return buf, kp, vp


def decode_legal(dc):
    """-> (Legal of the q heads [B, nq, hd], Legal of the K pool rows [B, nkv * dp], the V pool rows [B, nkv * dp] exactly)."""
    q = dc.qk
    L = qk_legal(q)
    B, nq, nkv, hd, dp = q.rows, q.nq, q.nkv, q.hd, q.dp

    def krows(t):
        r = torch.zeros(B, nkv, dp, dtype=BF16)
        r[:, :, :hd] = t[:, nq:]
        return r.reshape(B, -1)
    Lq = Legal(cands=[c[:, :nq] for c in L.cands])
    Lk = Legal(cands=[krows(c) for c in L.cands])
    v = torch.zeros(B, nkv, dp, dtype=BF16)
    v[:, :, :hd] = q.vheads()[:, :, :hd]
    return Lq, Lk, Legal(cands=[v.reshape(B, -1)])


def check_decode(dc, got, what=""):
    """got = (qkv buffer, K pool, V pool) -> the ambiguous share of q and K."""
    Lq, Lk, Lv = decode_legal(dc)
    order = dc.prow.argsort()                                       # ``check`` walks the region in row-major order
    q = dc.qk
    base = q.qkv0.clone()                                           # the k / v heads of the projection row are scratch once they are in the pools
    base[:q.rows, q.nq * q.dp:(q.nq + 2 * q.nkv) * q.dp] = got[0][:q.rows, q.nq * q.dp:(q.nq + 2 * q.nkv) * q.dp]
    s1 = check(dc.name + " q", got[0], base, dc.q_region, Lq, what)
    s2 = check(dc.name + " K pool", got[1], dc.pool0, dc.pool_region, Legal(cands=[c[order] for c in Lk.cands]), what)
    check(dc.name + " V pool", got[2], dc.pool0, dc.pool_region, Legal(cands=[c[order] for c in Lv.cands]), what)
    return max(s1, s2)


def decode_passes(dc, got):
    try:
        check_decode(dc, got)
        return True
    except AssertionError:
        return False


def run_decode(ops, dc, dev="cuda"):
    q = dc.qk
    buf, kp, vp = q.qkv0.to(dev).clone(), dc.pool0.to(dev).clone(), dc.pool0.to(dev).clone()
    w = [None if (t is None or not q.use_norm) else t.to(dev) for t in q.w]
    ops.decode_qkv_post(buf[:q.rows], q.cos.to(dev), q.sin.to(dev), w[0], w[1], kp, vp, dc.block_table.to(dev), dc.kv_len.to(dev), q.rows, q.nq, q.nkv,
                        q.hd, q.dp, q.eps, q.use_norm)
    return buf.cpu(), kp.cpu(), vp.cpu()


# ------------------------------------------------------------------------------------------------------------
# rope2d
# ------------------------------------------------------------------------------------------------------------
class Rope2dCase:
    """qkv0 [rows + 1, ld]: ``nheads`` q + k heads of dp lanes (values in [0, hd), SENTINEL pads), then V heads and trailing columns of SENTINEL.
    tables = (cos_h, sin_h, cos_w, sin_w) [P, hd / 2]; pos_ids [rows]: a permutation with repeats of table rows, not the row index."""

    def __init__(self, kind, rows, nheads, hd, dp, seed=0):
        g = _gen(30, seed, rows, nheads, hd)
        self.rows, self.nheads, self.hd, self.dp = rows, nheads, hd, dp
        P = rows + 5
        if kind == "tables":
            x = torch.randint(-127, 128, (rows, nheads, hd), generator=g).float().to(BF16)
            t = [designed_tables(P, hd // 2, k) for k in (0, 1)]
            self.tables = (t[0][0], t[0][1], t[1][0], t[1][1])
            assert len({bits(t).numpy().tobytes() for t in self.tables}) == 4
        else:
            x = (3 * torch.randn(rows, nheads, hd, generator=g)).to(BF16)
            inv = inv_freq(hd // 2, 1e4)                             # RotaryEmbedding2D: dim = hd / 2 per axis
            side = int(math.isqrt(P - 1)) + 1
            gh, gw = (torch.arange(P) // side).float(), (torch.arange(P) % side).float()
            fh, fw = gh[:, None] * inv[None], gw[:, None] * inv[None]
            eh, ew = torch.cat([fh, fh], -1), torch.cat([fw, fw], -1)
            self.tables = tuple(t.to(BF16).contiguous() for t in (eh.cos(), eh.sin(), ew.cos(), ew.sin()))
        pos = torch.rand(P, generator=g).argsort()[:rows]
        if rows >= 3:
            pos[rows // 2] = pos[0]                                    # a repeat
        self.pos_ids = pos.long()
        assert rows < 3 or not torch.equal(self.pos_ids, torch.arange(rows))
        self.name = f"rope2d {kind} rows {rows} heads {nheads} hd {hd}/{dp}"
        ld = (nheads + nheads // 2 + 1) * dp + 8
        buf = torch.full((rows + 1, ld), SENTINEL, dtype=BF16)
        heads = torch.full((rows, nheads, dp), SENTINEL, dtype=BF16)
        heads[:, :, :hd] = x
        buf[:rows, :nheads * dp] = heads.reshape(rows, -1)
        self.qkv0 = buf
        reg = torch.zeros(rows, nheads, dp, dtype=torch.bool)
        reg[:, :, :hd] = True
        self.region = torch.zeros(buf.shape, dtype=torch.bool)
        self.region[:rows, :nheads * dp] = reg.reshape(rows, -1)

    def heads(self):
        return self.qkv0[:self.rows, :self.nheads * self.dp].reshape(self.rows, self.nheads, self.dp)[:, :, :self.hd]


ROPE2D_MUTANTS = ("hw_swapped", "partner_h2", "pos_ignored", "k_skipped")


def emu_rope2d(case, mutant=None):
    """-> (the qkv buffer after an honest rope2d, the [rows, nheads, hd] results)."""
    rows, nh, hd, dp = case.rows, case.nheads, case.hd, case.dp
    h2, q4 = hd // 2, hd // 4
    x = case.heads().float()
    pos = torch.arange(rows) if mutant == "pos_ignored" else case.pos_ids
    ch, sh, cw, sw = (t[pos].float()[:, None, :] for t in case.tables)
    if mutant == "hw_swapped":
        ch, sh, cw, sw = cw, sw, ch, sh
    out = torch.empty_like(x)
    if mutant == "partner_h2":                                        # rotate-half over the whole head, each half with its own tables
        c, s = torch.cat([ch[..., :q4], ch[..., :q4], cw[..., :q4], cw[..., :q4]], -1), torch.cat([sh[..., :q4], sh[..., :q4], sw[..., :q4], sw[..., :q4]], -1)
        out = _bf(x * c) + _bf(_rot(x) * s)
    else:
        for half, (c, s) in enumerate(((ch, sh), (cw, sw))):
            xx = x[..., half * h2:(half + 1) * h2]
            out[..., half * h2:(half + 1) * h2] = _bf(xx * c) + _bf(_rot(xx) * s)
    out = out.to(BF16)
    if mutant == "k_skipped":
        out[:, nh // 2:] = case.heads()[:, nh // 2:]
    buf = case.qkv0.clone()
    hv = buf[:rows, :nh * dp].reshape(rows, nh, dp).clone()
    hv[:, :, :hd] = out
    buf[:rows, :nh * dp] = hv.reshape(rows, -1)
    return buf, out


def run_rope2d(ops, case, dev="cuda"):
    buf = case.qkv0.to(dev).clone()
    ops.rope2d(buf[:case.rows], tuple(t.to(dev) for t in case.tables), case.pos_ids.to(dev), case.nheads, case.hd, case.dp)
    return buf.cpu()
