"""Float64 reference, per-element error bound, fp32 emulation (+ wrong variants) and designed inputs for the attention forward kernels.
Pure torch on the CPU; tests/test_attn_ref_cpu.py validates it, tests/test_attn_numerics_gpu.py applies it to the HIP kernels.

A problem (``Problem``) is packed varlen attention in the layout of ``ops.attn_varlen``: bf16 q [M, nq, D], new k / v [M, nkv, D], context
k / v [Ctot, nkv, D], per-sample lengths, GQA by head groups, causal over the NEW keys only (a context key is visible to every row).
A row's keys are ordered context then new -- the order of the kernels' 64-key tile list [context tiles | new tiles].

THE BOUND  (eps = 2^-24, the fp32 unit roundoff; u = 2^-8, the bf16 half spacing relative to the value)

With p_j = exp2(z_j - max z), z_j = scale_log2 * s_j, l = sum_j p_j, ref = sum_j p_j v_j / l and A = sum_j p_j |v_j| / l a kernel returns
bf16(x) with

    |x - ref| <= (u + slack32) * A / (1 - u - slack32)            and so          |got - ref| <= e + u * (|ref| + e),   e = that right side.

To first order this is  u |ref| + u A + slack32 A;  the closed form adds only its second-order terms (the quotient by an l that is itself
off by u + slack32, and the output rounding applied to x instead of ref): a factor of about 1 + 2u.

  u * A      P is rounded to bf16 in front of the PV MFMA (attention.hip `pw[qbv][pi] = pack2bf(p0, p1)`; decode.hip `pfrag = {pack2bf(..`)
             while l sums the unrounded fp32 p (attention.hip `acc[..] += p0`, decode.hip `ls += pw[blk][r]`): the numerator carries a
             relative error <= u per term that the denominator does not share.
  u * (..)   the one output rounding (`pack2bf(o[..] * inv, ..)`).
  slack32    fp32 terms only, each a relative error of a term of the numerator (against A) or of l (against |ref| <= A):
      E_z = (D + 5) eps smax ln2    the exponent.  The score is an fp32 MFMA sum of D exact products (`sn[qb][kb] = ..mfma_f32_32x32x16_bf16`):
                                    <= D eps sum_d |q_d k_jd|; scale_log2 is an fp32 product of two rounded constants (`p.scale_log2 =
                                    softmax_scale * 1.4426950408889634f`): 2 eps |z|; `fmaf(sc, p.scale_log2, -m_use)` rounds once, at a
                                    magnitude <= 2 smax: 2 eps smax; one spare eps for decode.hip, which rounds `sacc * scale_log2e` and
                                    `sc - m_new` separately.  smax = max_j sum_d |q_d k_jd| scale_log2 bounds every |z|; an error dz of the
                                    exponent is a relative error ln2 dz of p.
      e_exp                         the exponential itself: v_exp_f32 (`__builtin_amdgcn_exp2f`) is good to 1 ulp = 2 eps; decode.hip
                                    calls `exp2f`: 4 eps.
      R (2 ln2 smax eps + e_exp + eps)   the rescale products.  Each raise of the running max multiplies O and l by alpha = exp2(m_run - m_new)
                                    (`raise_max`: `l_run[qb] *= alpha; o[qb][i][r] *= alpha`): the subtraction rounds at <= 2 smax, the
                                    exponential, one product.  Terms added later do not carry it, so it does not cancel.  R <= the number of
                                    64-key tiles T = ceil(n / 64) + 2 (a ragged context tile and a ragged new tile); decode.hip rescales
                                    once per 128-key chunk and once per merge level (wave merge, split loop, group merge): ceil(n / 128) + 3.
      E_p = E_z + e_exp + R (..)    every term of O and of l.
      n eps                         accumulation over the row's n keys, once for l (`acc[]`, `l_run +=`, the half-wave sum) and once for O
                                    (the PV MFMA chain).
      comb = 2 ln2 smax eps + 5 eps + T eps     one more fp32 sum, the key-split combine (attention2.hip `attn2_combine_kernel`:
                                    `w = exp2f(m - M)`, `den += w * ..`, `a[..] += v[..] * w` over <= T slots).  Only in the bound of
                                    the planned kernel; decode.hip's merges are counted in its R.
      3 eps                         `inv = 1.0f / l_tot` (2 eps) and the product with it.
    slack32 = 2 E_p + 2 n eps + 3 eps  (+ 2 comb for the planned kernel).
  One variant per kernel, ``kind``: "tile" (attention.hip: attn_varlen and the ranges / lse entries), "planned" (attention2.hip: tile +
  comb), "decode" (decode.hip: exp2f, its own R, no deferred maximum).
  Keys whose p underflows (z_j < max z - 126) are dropped by the kernels (and by a combine weight `exp2f(m - M)` = 0): each is a
  relative 2^-126 of the largest term, n 2^-126 in all -- far below eps and covered by the spare terms above.
Nothing here is fitted: with randn inputs at D = 128 and 500 keys slack32 is about 1e-4 against u = 3.9e-3; on the staircase inputs
(smax ~ 200) it reaches 1e-3.

The deferred maximum (P <= 2^8 relative to the maximum in use) changes no term: a relative error stays relative.

THE LSE BOUND (log2 units).  attention.hip writes `m_use + log2f(l_tot)`, l the fp32 sum of the UNROUNDED p (the bf16 rounding happens in
`pack2bf`, after `acc[] += p0`), so l carries delta = E_p + n eps and
    |lse - lse2| <= log2(1 + delta) + 4 eps (smax + log2 n + 8 + |lse2|)
(log2f to 2 ulp and the sum, at magnitudes <= smax resp. log2 n + 8 for a deferred maximum).  No u term: a kernel that summed bf16(p)
would be off by up to log2(1 + u) = 5.6e-3 on the `pbias` inputs below and fails this bound.

KEYSET inputs are checked exactly instead (``assert_keyset_exact``): q = 0 makes every p = 1, l = n and the per-dimension counts exact
integers in fp32, the combine weights exp2f(0) = 1, so x = count * (1 / n) within 3 eps and bf16(x) is one of the two bf16 neighbours of
count / n (the value itself when it is representable) -- that much is allowed and no more.

EMULATION.  ``emulate`` restates the kernels' algorithm in fp32 torch with the same rounding points (64-key tiles, base-2 online softmax, the
maximum raised per 32-row wave only when a row exceeds it by more than 2^8, bf16 P, fp32 l, optional key-split partials + combine) in
another summation order; ``MUTANTS`` are the ways it can be made subtly wrong.
"""
import math

import torch

BF16 = torch.bfloat16
EPS = 2.0 ** -24
U = 2.0 ** -8
LOG2E = 1.4426950408889634
DEFER_LOG2 = 8.0


class Problem:
    def __init__(self, q, k, v, kc, vc, q_lens, ctx_lens, causal, scale, name=""):
        self.q, self.k, self.v, self.kc, self.vc = q, k, v, kc, vc
        self.q_lens, self.ctx_lens = list(q_lens), list(ctx_lens)
        self.causal, self.scale, self.name = bool(causal), float(torch.tensor(scale, dtype=torch.float32)), name
        self.M, self.nq, self.D = q.shape
        self.nkv = k.shape[1]
        self.cu_q = [0]
        for n in self.q_lens:
            self.cu_q.append(self.cu_q[-1] + n)
        self.cu_c = [0]
        for n in self.ctx_lens:
            self.cu_c.append(self.cu_c[-1] + n)
        assert self.cu_q[-1] == self.M and all(t.dtype == BF16 for t in (q, k, v, kc, vc))

    def sample(self, b, dtype):
        """(q [Lq, nq, D], K [n, nq, D], V [n, nq, D], C) of sample b: keys context then new, KV heads repeated over their group."""
        q0, c0, Lq, C = self.cu_q[b], self.cu_c[b], self.q_lens[b], self.ctx_lens[b]
        G = self.nq // self.nkv
        K = torch.cat([self.kc[c0:c0 + C], self.k[q0:q0 + Lq]]).to(dtype).repeat_interleave(G, dim=1)
        V = torch.cat([self.vc[c0:c0 + C], self.v[q0:q0 + Lq]]).to(dtype).repeat_interleave(G, dim=1)
        return self.q[q0:q0 + Lq].to(dtype), K, V, C

    def visible(self, b):
        """bool [Lq, n]: row i sees every context key and the new keys <= i (causal) or all of them."""
        Lq, C = self.q_lens[b], self.ctx_lens[b]
        j = torch.arange(C + Lq)[None, :]
        i = torch.arange(Lq)[:, None]
        return (j < C) | (j - C <= i) if self.causal else torch.ones(Lq, C + Lq, dtype=torch.bool)


# ------------------------------------------------------------------------------------------------------------
# float64 reference and the bound
# ------------------------------------------------------------------------------------------------------------
def attn_ref(P):
    """-> refpack: ref / A [M, nq, D], lse2 / smax [M, nq], nkeys / sample / row [M], all float64 / int64."""
    sl2 = P.scale * LOG2E
    ref, A, lse2, smax, nk, sm, rw = [], [], [], [], [], [], []
    for b in range(len(P.q_lens)):
        q, K, V, _ = P.sample(b, torch.float64)
        vis = P.visible(b)
        z = torch.einsum("ihd,jhd->ihj", q, K) * sl2
        za = torch.einsum("ihd,jhd->ihj", q.abs(), K.abs()) * sl2
        z = z.masked_fill(~vis[:, None, :], -math.inf)
        m = z.max(-1, keepdim=True).values
        p = torch.exp2(z - m)
        l = p.sum(-1, keepdim=True)
        ref.append(torch.einsum("ihj,jhd->ihd", p, V) / l)
        A.append(torch.einsum("ihj,jhd->ihd", p, V.abs()) / l)
        lse2.append((m + torch.log2(l))[..., 0])
        smax.append(za.masked_fill(~vis[:, None, :], 0.0).max(-1).values)
        nk.append(vis.sum(1))
        sm.append(torch.full((P.q_lens[b],), b))
        rw.append(torch.arange(P.q_lens[b]))
    cat = torch.cat
    return dict(ref=cat(ref), A=cat(A), lse2=cat(lse2), smax=cat(smax), nkeys=cat(nk), sample=cat(sm), row=cat(rw), D=P.D)


def slack32(nkeys, smax, D, kind="tile"):
    """[M, nq] fp32-only relative slack and the relative error of l (the module docstring derives every term)."""
    n = nkeys.double()[:, None]
    ln2 = math.log(2.0)
    T = torch.ceil(n / 64) + 2
    if kind in ("tile", "planned"):
        e_exp, R = 2 * EPS, T
    elif kind == "decode":
        e_exp, R = 4 * EPS, torch.ceil(n / 128) + 3
    else:
        raise ValueError(kind)
    E_z = (D + 5) * EPS * smax * ln2
    E_p = E_z + e_exp + R * (2 * ln2 * smax * EPS + e_exp + EPS)
    comb = (2 * ln2 * smax * EPS + 5 * EPS + T * EPS) if kind == "planned" else 0.0
    return 2 * E_p + 2 * n * EPS + 2 * comb + 3 * EPS, E_p + n * EPS


def attn_bound(rp, kind="tile"):
    s, _ = slack32(rp["nkeys"], rp["smax"], rp["D"], kind)
    e = (U + s)[..., None] * rp["A"] / (1 - U - s)[..., None]
    return e + U * (rp["ref"].abs() + e)


def lse_bound(rp, kind="tile"):
    _, delta = slack32(rp["nkeys"], rp["smax"], rp["D"], kind)
    n = rp["nkeys"].double()[:, None]
    return torch.log2(1 + delta) + 4 * EPS * (rp["smax"] + torch.log2(n) + 8 + rp["lse2"].abs())


def _worst(err, bound, rp, names):
    ratio = err / bound.clamp_min(1e-300)
    ratio = torch.where((err == 0) & (bound == 0), torch.zeros_like(ratio), ratio)
    idx = ratio.argmax().item()
    pos = []
    for s in reversed(err.shape):
        pos.append(idx % s)
        idx //= s
    pos = pos[::-1]
    where = f"sample {int(rp['sample'][pos[0]])} row {int(rp['row'][pos[0]])} " + " ".join(f"{n} {p}" for n, p in zip(names, pos[1:]))
    return ratio.max().item(), where, tuple(pos)


def attn_ratio(got, rp, kind="tile"):
    """worst err / bound (inf for a non-finite output), where, index -- no assertion."""
    got = got.detach().cpu().double()
    assert got.shape == rp["ref"].shape, (got.shape, rp["ref"].shape)
    err = (got - rp["ref"]).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, math.inf))
    return _worst(err, attn_bound(rp, kind), rp, ("head", "dim"))


def assert_attn_close(got, rp, what, kind="tile"):
    """Every element within its own bound; -> the worst err / bound.  No whole-tensor scale anywhere."""
    ratio, where, pos = attn_ratio(got, rp, kind)
    if not ratio <= 1.0:
        g, r = got.detach().cpu().double()[pos].item(), rp["ref"][pos].item()
        raise AssertionError(f"{what}: err / bound = {ratio:.3f} at {where}: got {g!r} ref {r!r} "
                             f"(A {rp['A'][pos].item():.4g}, {int(rp['nkeys'][pos[0]])} keys, smax {rp['smax'][pos[:2]].item():.4g})")
    return ratio


def lse_ratio(lse, rp, kind="tile"):
    lse = lse.detach().cpu().double()
    err = (lse - rp["lse2"]).abs()
    err = torch.where(torch.isfinite(lse), err, torch.full_like(err, math.inf))
    return _worst(err, lse_bound(rp, kind), rp, ("head",))


def assert_lse_close(lse, rp, what, kind="tile"):
    """lse [M, nq] (log2 of the softmax denominator in the scaled base-2 domain) within its bound; -> worst err / bound."""
    ratio, where, pos = lse_ratio(lse, rp, kind)
    if not ratio <= 1.0:
        raise AssertionError(f"{what}: lse err / bound = {ratio:.3f} at {where}: got {lse.detach().cpu()[pos].item()!r} ref {rp['lse2'][pos].item()!r}")
    return ratio


def _bf16_neighbours(r):
    """(largest bf16 <= r, smallest bf16 >= r) for float64 r >= 0."""
    b = r.float().to(BF16)
    bits = b.view(torch.int16).to(torch.int32)
    up = (bits + 1).to(torch.int16).view(BF16).double()
    dn = torch.where(bits > 0, bits - 1, bits).to(torch.int16).view(BF16).double()
    bd = b.double()
    lo = torch.where(bd <= r, bd, dn)
    hi = torch.where(bd >= r, bd, up)
    return lo, hi


def keyset_counts(P):
    """(count [M, nq, D], n [M]) of a keyset problem: count[i, h, d] = visible keys of row i whose one-hot V sits at dimension d."""
    cnt, ns = [], []
    for b in range(len(P.q_lens)):
        _, _, V, _ = P.sample(b, torch.float64)
        vis = P.visible(b).double()
        cnt.append(torch.einsum("ij,jhd->ihd", vis, V))
        ns.append(vis.sum(1))
    return torch.cat(cnt), torch.cat(ns)


def keyset_ratio(got, P):
    """(0.0 if every output is a bf16 neighbour of count / n else inf, flat index of the element farthest outside) -- pass or fail, there
    is no meaningful ratio for an exact check."""
    cnt, n = keyset_counts(P)
    lo, hi = _bf16_neighbours(cnt / n[:, None, None])
    g = got.detach().cpu().double()
    ok = torch.isfinite(g) & ((g == lo) | (g == hi))
    off = torch.where(torch.isfinite(g), torch.maximum(lo - g, g - hi).clamp_min(0), torch.full_like(g, math.inf))
    off = torch.where(ok, torch.zeros_like(off), off)
    return (0.0 if bool(ok.all()) else math.inf), off.argmax().item()


def assert_keyset_exact(got, P, what):
    ratio, idx = keyset_ratio(got, P)
    if ratio != 0.0:
        cnt, n = keyset_counts(P)
        i, h, d = idx // (P.nq * P.D), idx // P.D % P.nq, idx % P.D
        raise AssertionError(f"{what}: packed row {i} head {h} dim {d}: got {got.detach().cpu().double()[i, h, d].item()!r}, "
                             f"expected a bf16 neighbour of {int(cnt[i, h, d])} / {int(n[i])} (a key dropped, added or mis-weighted)")
    return ratio


# ------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernels and its wrong variants
# ------------------------------------------------------------------------------------------------------------
MUTANTS = ("drop_key", "diag_plus", "diag_minus", "tail_extra", "leak_next", "swap_s", "rescale_skipped", "rescale_l_only", "comb_weight_one",
           "round_p_before_sum")


def _f32(x):
    return x.to(torch.float32)


def emulate(P, splits=1, mutant=None):
    """-> (out bf16 [M, nq, D], lse fp32 [M, nq]).  ``splits`` > 1: the tile list of every sample is cut into that many contiguous ranges
    (where it has the tiles), each leaves an fp32 partial (O, maximum in use, l) and the combine of attention2.hip merges them.
    ``mutant``: one of MUTANTS, always applied to sample 0 (see the branches below)."""
    assert mutant is None or mutant in MUTANTS
    sl2 = torch.tensor(P.scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    outs, lses = [], []
    for b in range(len(P.q_lens)):
        q, K, V, C = P.sample(b, torch.float32)
        Lq, nq = P.q_lens[b], P.nq
        n = C + Lq
        vis = P.visible(b).clone()
        mut = mutant if b == 0 else None
        Ks = K                                            # what the score side reads
        # two ghost keys behind the new segment: the clamped re-read of the last key with the zero V^T pad column behind it, and the
        # next sample's first new key with its V; visible only to the mutants that admit them
        G = nq // P.nkv
        nxt = P.cu_q[b + 1] if b + 1 < len(P.q_lens) else None
        ghostK = [K[-1:], _f32(P.k[nxt:nxt + 1]).repeat_interleave(G, dim=1) if nxt is not None else K[-1:]]
        ghostV = [torch.zeros_like(V[-1:]), _f32(P.v[nxt:nxt + 1]).repeat_interleave(G, dim=1) if nxt is not None else torch.zeros_like(V[-1:])]
        Ks, V = torch.cat([Ks] + ghostK), torch.cat([V] + ghostV)
        vis = torch.cat([vis, torch.zeros(Lq, 2, dtype=torch.bool)], 1)
        blk = slice(max(Lq - 32, 0), Lq)                  # the last 32-row wave of the sample
        if mut == "drop_key":                             # one key of one row: the middle key of the last row's set
            vis[Lq - 1, n // 2] = False
        elif mut in ("diag_plus", "diag_minus") and P.causal:
            i = torch.arange(Lq)[:, None]
            jn = torch.arange(Lq)[None, :]
            d = 1 if mut == "diag_plus" else -1
            rows = slice(max(Lq // 2, 1), max(Lq // 2, 1) + 32)
            vis[rows, C:n] = (jn <= i + d)[rows]
        elif mut == "tail_extra":
            vis[blk, n] = True
        elif mut == "leak_next" and nxt is not None:
            vis[blk, n + 1] = True
        elif mut == "swap_s" and Lq >= 5:                 # new keys 0 and 4 (quads 0 and 1 of one 16-key group) trade places for S only
            Ks = Ks.clone()
            Ks[[C, C + 4]] = Ks[[C + 4, C]]
        elif mut == "swap_s" and C >= 6:                  # a one-row (decode) sample: context keys 1 and 5
            Ks = Ks.clone()
            Ks[[1, 5]] = Ks[[5, 1]]
        # the tile list: context tiles, then new tiles (the ghosts ride in the last one)
        tiles = [(t, min(t + 64, C)) for t in range(0, C, 64)] + [(C + t, C + min(t + 64, Lq)) for t in range(0, Lq, 64)]
        tiles[-1] = (tiles[-1][0], n + 2)
        S = max(1, min(splits, len(tiles)))
        cuts = [round(i * len(tiles) / S) for i in range(S + 1)]
        parts = []
        for s in range(S):
            o = torch.zeros(Lq, nq, P.D)
            l = torch.zeros(Lq, nq)
            m_run = torch.full((Lq, nq), -math.inf)
            m_use = torch.zeros(Lq, nq)
            for (j0, j1) in tiles[cuts[s]:cuts[s + 1]]:
                sc = torch.einsum("ihd,jhd->ihj", q, Ks[j0:j1]).masked_fill(~vis[:, None, j0:j1], -math.inf)
                mx = sc.max(-1).values * sl2
                grow = mx > m_run + DEFER_LOG2
                pad = (-Lq) % 32                          # `__any(grow)`: the 32 rows of a wave raise their maxima together
                gw = torch.cat([grow, torch.zeros(pad, nq, dtype=torch.bool)]).view(-1, 32, nq).any(1)
                grow = gw.repeat_interleave(32, dim=0)[:Lq]
                m_new = torch.where(grow, torch.maximum(m_run, mx), m_run)
                fin = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
                alpha = torch.where(grow, torch.exp2(m_run - fin), torch.ones_like(m_run))
                m_use = torch.where(grow, fin, m_use)
                m_run = m_new
                if mut == "rescale_skipped":
                    pass
                elif mut == "rescale_l_only":
                    l = l * alpha
                else:
                    l = l * alpha
                    o = o * alpha[..., None]
                p = torch.exp2((sc.double() * sl2.double() - m_use.double()[..., None]).float())      # the fma: one rounding
                pb = p.to(BF16).float()
                l = l + (pb if mut == "round_p_before_sum" else p).sum(-1)
                o = o + torch.einsum("ihj,jhd->ihd", pb, V[j0:j1])
            parts.append((o, torch.where(torch.isinf(m_run), m_run, m_use), l))
        if S == 1:
            o, m, l = parts[0]
            outs.append((o * (1.0 / l)[..., None]).to(BF16))
            lses.append(m + torch.log2(l))
        else:
            Mx = torch.stack([p[1] for p in parts]).max(0).values
            den = torch.zeros(Lq, nq)
            a = torch.zeros(Lq, nq, P.D)
            for o, m, l in parts:
                w = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - Mx))
                if mut == "comb_weight_one":
                    w = torch.where(torch.isinf(m), w, torch.ones_like(w))
                den = den + w * l
                a = a + o * w[..., None]
            outs.append((a * (1.0 / den)[..., None]).to(BF16))
            lses.append(Mx + torch.log2(den))
    return torch.cat(outs), torch.cat(lses)


# ------------------------------------------------------------------------------------------------------------
# designed inputs
# ------------------------------------------------------------------------------------------------------------
def _rnd(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF16)


def _key_index(q_lens, ctx_lens):
    """index of every key inside its own row set (context then new): (context [Ctot], new [M]) and the tile it lies in."""
    ci, ni, ct, nt = [], [], [], []
    for Lq, C in zip(q_lens, ctx_lens):
        ci.append(torch.arange(C)); ni.append(C + torch.arange(Lq))
        ct.append(torch.arange(C) // 64); nt.append((C + 63) // 64 + torch.arange(Lq) // 64)
    return torch.cat(ci), torch.cat(ni), torch.cat(ct), torch.cat(nt)


def _onehot(idx, nkv, D):
    v = torch.zeros(len(idx), nkv, D)
    v[torch.arange(len(idx)), :, idx % D] = 1.0
    return v.to(BF16)


def _pbias_beta():
    """beta = k / 64 in [1, 4) (exact in bf16) whose p = 2^-(beta^2) has the largest bf16 rounding error relative to p, rounding DOWN."""
    best, arg = 0.0, None
    for k in range(64, 256):
        L = (k / 64.0) ** 2
        if not 2.0 <= L <= 7.0:
            continue
        p = torch.tensor(2.0 ** -L, dtype=torch.float64)
        rel = ((p - p.float().to(BF16).double()) / p).item()
        if rel > best:
            best, arg = rel, k / 64.0
    return arg


FAMILIES = ("keyset", "pairing4", "pairing12", "peaked4", "peaked8", "stair6", "stair20", "stair_down", "split136", "split3", "sink", "pbias")


def build(family, q_lens, ctx_lens, nq, nkv, D, causal, seed=0):
    """A seeded problem of one designed family:
      keyset        q = 0, V one-hot at (key index mod D): every p is 1, an output is count / n -- pins the key set of every row;
      pairing4/12   k_j = beta e_(j mod D), q_i = beta e_(hot key of row i), V one-hot: weight 2^4 (below the deferral threshold) or 2^12
                    (above it) sits on the hot key's dimension -- pins the key order of S against that of V^T;
      peaked4/8     randn with q scaled by 4 / 8;
      stair6/20/_down   the row maximum climbs 6 (two tiles pass the deferral threshold together) or 20 per 64-key tile, or falls by 6;
      split136/3    the first half of the tile list scores 136 (a combine weight underflows to 0) or 3 log2 units above the second;
      sink          one key (the first of every row set) 30 log2 units above randn scores;
      pbias         the pairing layout with a score gap whose p = 2^-gap rounds to bf16 with a near-maximal one-sided error, which
                    separates a sum of rounded p from a sum of unrounded p in the lse."""
    g = torch.Generator().manual_seed(1000 * seed + FAMILIES.index(family))
    M, Ct = sum(q_lens), sum(ctx_lens)
    ci, ni, ct, nt = _key_index(q_lens, ctx_lens)
    scale = D ** -0.5
    q, k, v, kc, vc = _rnd(g, M, nq, D), _rnd(g, M, nkv, D), _rnd(g, M, nkv, D), _rnd(g, Ct, nkv, D), _rnd(g, Ct, nkv, D)
    if family == "keyset":
        q = torch.zeros_like(q)
        v, vc = _onehot(ni, nkv, D), _onehot(ci, nkv, D)
    elif family in ("pairing4", "pairing12", "pbias"):
        beta = _pbias_beta() if family == "pbias" else 2.0
        L = {"pairing4": 4.0, "pairing12": 12.0}.get(family)
        scale = (1.0 if family == "pbias" else L / beta ** 2) / LOG2E          # beta^2 * scale_log2 = L  (pbias: beta^2)
        k, kc = (_onehot(ni, nkv, D).float() * beta).to(BF16), (_onehot(ci, nkv, D).float() * beta).to(BF16)
        v, vc = _onehot(ni, nkv, D), _onehot(ci, nkv, D)
        # hot key of row i, cycling: first tile, an interior tile, the ragged last tile, the context, the new keys (visible under causal)
        q = torch.zeros(M, nq, D)
        r0 = 0
        for Lq, C in zip(q_lens, ctx_lens):
            n = C + Lq
            hot = [1, (n // 128) * 64 + 7, n - 2, max(C - 3, 0), C]
            for i in range(Lq):
                for h in range(nq):
                    q[r0 + i, h, hot[(i + h) % 5] % n % D] = beta
            r0 += Lq
        q = q.to(BF16)
    elif family in ("peaked4", "peaked8"):
        q = (q.float() * (4.0 if family == "peaked4" else 8.0)).to(BF16)
    elif family in ("stair6", "stair20", "stair_down", "split136", "split3", "sink"):
        # dimension 0 carries a designed score on top of the randn ones: q_0 = 4, k_0 = level(key) / (4 * scale_log2)
        sl2 = scale * LOG2E
        if family.startswith("stair"):
            step = {"stair6": 6.0, "stair20": 20.0, "stair_down": -6.0}[family]
            lc, ln = step * ct.float(), step * nt.float()
        elif family.startswith("split"):
            gap = 136.0 if family == "split136" else 3.0
            half = torch.cat([torch.full((Lq,), ((C + 63) // 64 + (Lq + 63) // 64) // 2) for Lq, C in zip(q_lens, ctx_lens)])
            halfc = torch.cat([torch.full((C,), ((C + 63) // 64 + (Lq + 63) // 64) // 2) for Lq, C in zip(q_lens, ctx_lens)])
            lc, ln = gap * (ct < halfc).float(), gap * (nt < half).float()
        else:       # sink: the first key of every row set (context key 0, or new key 0 without a context)
            lc, ln = 30.0 * (ci == 0).float(), 30.0 * (ni == 0).float()
        q, k, kc = q.float(), k.float(), kc.float()
        q[:, :, 0] = 4.0
        k[:, :, 0] = (ln / (4.0 * sl2))[:, None]
        kc[:, :, 0] = (lc / (4.0 * sl2))[:, None]
        q, k, kc = q.to(BF16), k.to(BF16), kc.to(BF16)
    else:
        raise ValueError(family)
    return Problem(q, k, v, kc, vc, q_lens, ctx_lens, causal, scale, name=family)


# shapes of the GPU module: the smallest that reach two 256-row query tiles, a head-per-wave tail (<= 32 rows), >= 5 key tiles (the 3- and
# 4-slot rings wrap), ragged last tiles, contexts that end inside a tile, item seams between samples and key-split items
SHAPES = [([290, 1, 65], [70, 0, 200]), ([34], [0]), ([330], [133])]
HEADS = [(4, 2, 128), (7, 1, 128), (4, 2, 64)]

# paged decode: one query row per request; key counts on both sides of a 64-key page, a 128-key chunk and (two chunks per workgroup) a
# 256-key workgroup range
DEC_LENS = [63, 64, 65, 127, 128, 129, 255, 257, 300]
DEC_FAMILIES = ("keyset", "pairing4", "pairing12", "sink")


def build_decode(family, nq, nkv, D):
    """The decode problem of one family: request b attends to DEC_LENS[b] keys, the last of them its own new key."""
    return build(family, [1] * len(DEC_LENS), [n - 1 for n in DEC_LENS], nq, nkv, D, True)
