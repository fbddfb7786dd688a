"""Per-row numerics of the attention forward kernels: every kernel form on designed inputs against the float64 reference and the
per-element bound of tests/util_attn_ref.py (derived there from the number formats, validated on the CPU by tests/test_attn_ref_cpu.py).

Forms: the tile kernel (``attn_varlen``), the planned persistent kernel with the five plans of tests/test_attn2_gpu.py (``attn_planned``: chip
default, 8 workers, 16 workers with every partial round key-split, twice the chip's workers, the same with key splits), the ``ranges`` entry
with ``lse`` (training), and paged decode attention (``attn_decode_paged``, also with two chunks per workgroup in a child process).
Families: see ``util_attn_ref.build`` -- keyset (the key set of every row, checked exactly), pairing (key order of S against V^T), peaked,
staircase (the deferred maximum and its rescale), split (combine weights, one of them underflowing), sink, pbias (lse).
Every output buffer is NaN-filled, rows outside every range keep a sentinel, the V^T pad columns are checked to be zero, and every test
prints its worst err / bound per form.
"""
import os
import subprocess
import sys

import pytest
import torch

from tests import util_attn_ref as R
from tests.test_attn2_gpu import _unsplit_rows
from tests.test_ops_gpu import BF16, DEV, attention_device_inputs, ops

pytestmark = pytest.mark.gpu

PLANS = [("chip", dict()), ("w8", dict(n_workers=8)), ("w16_split", dict(n_workers=16, split_min_tiles=1)),
         ("oversubscribed", dict(n_workers="2xchip")), ("oversubscribed_keysplit", dict(n_workers="2xchip", split_min_tiles=1))]
PAD, GAP, SENTINEL = 3, 2, 7.0        # rows behind the last sample; rows in front of every sample in the ranges layout


def _check_vt_pads(vt, lens, col0, what):
    """V^T contract: the columns between a sample's last key and the end of its last 64-column block are zero."""
    vt = vt.cpu()
    for n, c in zip(lens, col0):
        end = c + (max(n, 1) + 63) // 64 * 64
        assert (vt[:, c + n:end] == 0).all(), f"{what}: V^T pad columns {c + n}..{end} must be zero"


def run_forms(P):
    """-> {form: out [M, nq, D] on the host}, lse [M, nq], plans {form: AttnPlan}.  Buffers carry PAD rows that no range covers; the ranges
    entry runs on a second layout of the same q / k rows with GAP rows in front of every sample (holes between its ranges)."""
    o = ops()
    nq, nkv, D, M = P.nq, P.nkv, P.D, P.M
    B = len(P.q_lens)
    dv = attention_device_inputs(P.q, P.k, P.v, P.kc, P.vc, P.q_lens, P.ctx_lens, nq, nkv, D, pad_rows=PAD)
    qkv, vt, i32, kwargs = dv["qkv"], dv["vt"], dv["i32"], dv["kwargs"]
    qw, kw = nq * D, nkv * D
    has_ctx = bool(kwargs)
    _check_vt_pads(vt, P.q_lens, dv["vcol"], "new")
    if has_ctx:
        _check_vt_pads(dv["vtc"], P.ctx_lens, dv["ccol"], "context")

    def fresh():
        out = torch.full((M + PAD, qw), float("nan"), dtype=BF16, device=DEV)
        out[M:] = SENTINEL
        return out

    def done(out, what):
        assert (out[M:] == SENTINEL).all(), f"{what}: rows outside every range were written"
        return out[:M].cpu().view(M, nq, D)
    outs, plans = {}, {}
    out = fresh()
    o.attn_varlen(qkv[:, :qw], qkv[:, qw:qw + kw], vt, out, i32(dv["cu_q"]), i32(dv["vcol"]), B, max(P.q_lens), nq, nkv, D, P.causal, P.scale, **kwargs)
    outs["varlen"] = done(out, "attn_varlen")
    for name, plan in PLANS:
        if plan.get("n_workers") == "2xchip":
            plan = dict(plan, n_workers=2 * (torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8))
        ap = o.AttnPlan(dv["cu_q"][:-1], P.q_lens, dv["vcol"], nq, nkv, D, P.causal, DEV, ctx_start=dv["cu_c"][:-1] if has_ctx else None,
                        ctx_len=P.ctx_lens if has_ctx else None, vt_ctx_col=dv["ccol"] if has_ctx else None, **plan)
        out = fresh()
        o.attn_planned(qkv[:, :qw], qkv[:, qw:qw + kw], vt, out, ap, P.scale, k_ctx=kwargs.get("k_ctx"), vt_ctx=kwargs.get("vt_ctx"))
        outs[name], plans[name] = done(out, name), ap
    # ranges + lse: sample b's rows start at cu_q[b] + (b + 1) * GAP; V^T is addressed by column and stays as it is
    starts = [dv["cu_q"][b] + (b + 1) * GAP for b in range(B)]
    ends = [s + n for s, n in zip(starts, P.q_lens)]
    rows = torch.cat([torch.arange(s, e) for s, e in zip(starts, ends)]).to(DEV)
    Mg = M + B * GAP + PAD
    hole = torch.ones(Mg, dtype=torch.bool, device=DEV)
    hole[rows] = False
    qk_gap = torch.zeros((Mg, qw + kw), dtype=BF16, device=DEV)
    qk_gap[rows] = qkv[:M, :qw + kw]
    out = torch.full((Mg, qw), float("nan"), dtype=BF16, device=DEV)
    out[hole] = SENTINEL
    lse = torch.full((nq, Mg), float("nan"), dtype=torch.float32, device=DEV)
    lse[:, hole] = SENTINEL
    rk = dict(k_ctx=kwargs["k_ctx"], vt_ctx=kwargs["vt_ctx"], ctx_start=i32(dv["cu_c"][:-1]), ctx_end=i32(dv["cu_c"][1:]),
              vt_ctx_col=kwargs["vt_ctx_col"]) if has_ctx else {}
    o.attn_varlen_ranges(qk_gap[:, :qw], qk_gap[:, qw:], vt, out, i32(starts), i32(ends), i32(dv["vcol"]), B, max(P.q_lens),
                         nq, nkv, D, P.causal, P.scale, lse=lse, **rk)
    assert (out[hole] == SENTINEL).all(), "attn_varlen_ranges: rows outside every range (holes between ranges included) were written"
    assert (lse[:, hole] == SENTINEL).all(), "lse: columns outside every range were written"
    outs["ranges_lse"] = out[rows].cpu().view(M, nq, D)
    torch.cuda.synchronize()
    _check_vt_pads(vt, P.q_lens, dv["vcol"], "new (after the launches)")
    if has_ctx:
        _check_vt_pads(dv["vtc"], P.ctx_lens, dv["ccol"], "context (after the launches)")
    return outs, lse[:, rows].t().cpu(), plans


CASES = [(si, hi, causal) for si in range(len(R.SHAPES)) for hi in range(len(R.HEADS)) for causal in (True, False)]


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("si,hi,causal", CASES)
def test_attention_forms_on_designed_inputs(si, hi, causal, family):
    (ql, cl), (nq, nkv, D) = R.SHAPES[si], R.HEADS[hi]
    P = R.build(family, ql, cl, nq, nkv, D, causal)
    rp = R.attn_ref(P)
    outs, lse, plans = run_forms(P)
    what = f"{family} q={ql} ctx={cl} heads {nq}/{nkv} D={D} causal={causal}"
    ratios = {}
    for form, got in outs.items():
        if family == "keyset":
            ratios[form] = R.assert_keyset_exact(got, P, f"{what} [{form}]")
        else:
            ratios[form] = R.assert_attn_close(got, rp, f"{what} [{form}]", kind="planned" if form in plans else "tile")
    ratios["lse"] = R.assert_lse_close(lse, rp, f"{what} [ranges_lse]", kind="tile")
    print(f"{what}: worst err / bound " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    # the same launch arithmetic: the ranges entry is the tile kernel, and an un-split item of the planned kernel equals it bit for bit
    bits = lambda t: t.contiguous().view(torch.int16)  # noqa: E731
    assert torch.equal(bits(outs["ranges_lse"]), bits(outs["varlen"]))
    for form, ap in plans.items():
        keep = _unsplit_rows(ap, P.M, nq)
        a, b = bits(outs["varlen"])[keep], bits(outs[form])[keep]
        assert torch.equal(a, b), f"{what} [{form}]: un-split items must equal the tile kernel bit for bit ({int((a != b).any(-1).sum())} rows differ)"
    if si != 1:       # shapes with >= 5 key tiles: the key-split plans do split (the 34-row prompt has a single tile)
        assert plans["w16_split"].n_comb > 0 and plans["oversubscribed_keysplit"].n_comb > 0


# ------------------------------------------------------------------------------------------------------------
# paged decode attention
# ------------------------------------------------------------------------------------------------------------
DEC_LENS, DEC_FAMILIES = R.DEC_LENS, R.DEC_FAMILIES        # shared with the CPU validation of the decode bound


@pytest.mark.parametrize("family", DEC_FAMILIES)
@pytest.mark.parametrize("nq,nkv,D", R.HEADS)
def test_decode_attention_on_designed_inputs(nq, nkv, D, family):
    """One query row per request over its paged cache (the request's last key is its own new key): the decode variant of the bound
    (exp2f, one rescale per chunk and per merge level)."""
    from bagel_amd.modeling.bagel.decode import PagedKVCache
    o = ops()
    B = len(DEC_LENS)
    P = R.build_decode(family, nq, nkv, D)
    rp = R.attn_ref(P)
    width = nkv * D
    cap = max(DEC_LENS) + 3
    g = torch.Generator().manual_seed(7)
    order = torch.randperm(B * ((cap + 63) // 64), generator=g).tolist()          # physically scattered pages
    pg = PagedKVCache(1, B, width, cap, DEV, order=order)
    rows_k, rows_v = [], []
    for b in range(B):
        rows_k += [P.kc[P.cu_c[b]:P.cu_c[b + 1]], P.k[b:b + 1]]
        rows_v += [P.vc[P.cu_c[b]:P.cu_c[b + 1]], P.v[b:b + 1]]

    class FakeCache:       # what PagedKVCache.adopt reads from a NaiveCache: merged rows per layer
        _k = {0: torch.cat(rows_k).reshape(-1, width).to(DEV)}
        _v = {0: torch.cat(rows_v).reshape(-1, width).to(DEV)}
    pg.adopt(FakeCache, DEC_LENS)
    q = torch.cat([P.q.reshape(B, nq * D), torch.zeros(PAD, nq * D, dtype=BF16)]).to(DEV)
    worst = 0.0
    for max_len in (max(DEC_LENS), max(DEC_LENS) + 200):
        po, pml = o.attn_decode_workspace(B, nq, D, max_len, DEV)
        out = torch.full((B + PAD, nq * D), float("nan"), dtype=BF16, device=DEV)
        out[B:] = SENTINEL
        o.attn_decode_paged(q, pg.k[0], pg.v[0], pg.block_table, pg.kv_len, 0, max_len, po, pml, out, B, nq, nkv, D, P.scale)
        assert (out[B:] == SENTINEL).all(), "decode attention wrote rows past the batch"
        got = out[:B].cpu().view(B, nq, D)
        what = f"decode {family} heads {nq}/{nkv} D={D} max_len={max_len} cpw={os.environ.get('BAGEL_DEC_CPW', 'auto')}"
        worst = max(worst, R.assert_keyset_exact(got, P, what) if family == "keyset" else R.assert_attn_close(got, rp, what, kind="decode"))
    print(f"decode {family} heads {nq}/{nkv} D={D} cpw={os.environ.get('BAGEL_DEC_CPW', 'auto')}: worst err / bound {worst:.3f}")


def test_decode_attention_on_designed_inputs_with_two_chunks_per_workgroup():
    """The same cases with the chunk loop forced on (BAGEL_DEC_CPW is read once per process: a child process, as in tests/test_decode_gpu.py)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BAGEL_DEC_CPW="2")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-s", "-k",
                        "test_decode_attention_on_designed_inputs and not two_chunks"], env=env, capture_output=True, text=True, timeout=600, cwd=root)
    print("\n".join(l for l in r.stdout.splitlines() if "err / bound" in l))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
