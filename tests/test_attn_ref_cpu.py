"""The reference, bounds and designed inputs of tests/test_attn_numerics_gpu.py, validated without a GPU (tests/util_attn_ref.py).

An fp32 restatement of the attention kernels' algorithm (64-key tiles, base-2 online softmax with the deferred maximum, bf16 P, fp32 l,
key-split partials + combine; another summation order) must pass the per-element bound, the lse bound and the exact keyset check on every
family and shape the GPU module runs; restatements that are wrong in the ways the bounds are meant to catch must fail, and WHICH family
catches WHICH mutant is asserted (``CATCHES``).

What seeded randn data cannot catch (measured here, ``test_what_random_data_misses``):
  * a rescale that is skipped, or applied to l only, when the running maximum is raised: with scores ~ N(0, 1) no tile maximum exceeds the
    first tile's by 2^8, the branch never runs after the first tile;
  * P rounded to bf16 before the l sum: the rounding errors of ~uniform p average out (and the output even gets closer to the reference);
    only the lse of the `pbias` family, whose p all round the same way, shows it;
  * one dropped key among n uniform keys moves an output by about p_j |v_j| / l against a bound of about u A: err / bound depends on the
    weight of the key that happens to be dropped -- over eight seeds 0.3 .. 2.5 at 463 keys (printed) and 0.1 .. 0.7 at the product's
    4098 keys (asserted to stay under the bound).  The keyset family exists for this: there one key moves a count of at most 8 by 1.
"""
import pytest
import torch

from tests import util_attn_ref as R

BF16 = torch.bfloat16
CASES = [(si, hi, causal) for si in range(len(R.SHAPES)) for hi in range(len(R.HEADS)) for causal in (True, False)]


def _ratio(P, rp, out):
    return R.keyset_ratio(out, P)[0] if P.name == "keyset" else R.attn_ratio(out, rp)[0]


@pytest.mark.parametrize("si,hi,causal", CASES)
def test_emulation_passes_every_family(si, hi, causal):
    (ql, cl), (nq, nkv, D) = R.SHAPES[si], R.HEADS[hi]
    for fam in R.FAMILIES:
        P = R.build(fam, ql, cl, nq, nkv, D, causal)
        rp = R.attn_ref(P)
        res = {}
        for splits, kind in ((1, "tile"), (3, "planned")):        # un-split: the tile kernel's bound; key-split: the planned kernel's
            out, lse = R.emulate(P, splits=splits)
            if fam == "keyset":
                res[kind] = R.assert_keyset_exact(out, P, f"{fam} splits {splits}")
            else:
                res[kind] = R.assert_attn_close(out, rp, f"{fam} splits {splits}", kind=kind)
            res[kind + "_lse"] = R.assert_lse_close(lse, rp, f"{fam} splits {splits}", kind=kind)
        print(f"q {ql} ctx {cl} heads {nq}/{nkv} D {D} causal {causal} {fam:10s}: emulation err / bound " + " ".join(f"{k} {v:.3f}" for k, v in res.items()))


@pytest.mark.parametrize("family", R.DEC_FAMILIES)
@pytest.mark.parametrize("nq,nkv,D", R.HEADS)
def test_emulation_passes_the_decode_cases(nq, nkv, D, family):
    """The decode problems of the GPU module (one row per request, key counts on both sides of a page and a chunk) against the decode
    variant of the bound; a dropped key and an S-side key swap must fail there too."""
    P = R.build_decode(family, nq, nkv, D)
    rp = R.attn_ref(P)
    out, _ = R.emulate(P)
    if family == "keyset":
        r = R.assert_keyset_exact(out, P, f"decode {family}")
        assert R.keyset_ratio(R.emulate(P, mutant="drop_key")[0], P)[0] > 1.0, "a dropped key must fail the exact keyset check"
    else:
        r = R.assert_attn_close(out, rp, f"decode {family}", kind="decode")
    if family.startswith("pairing"):
        for mutant in ("drop_key", "swap_s"):
            rm = R.attn_ratio(R.emulate(P, mutant=mutant)[0], rp, kind="decode")[0]
            print(f"decode {family} {mutant}: err / bound = {rm:.1f}")
            assert rm > 1.0, f"{mutant} must fail the decode bound on {family}"
    print(f"decode {family} heads {nq}/{nkv} D {D}: emulation err / bound = {r:.3f}")


# mutant -> [(family, shape index, causal, "out" | "lse")]: every listed pair must FAIL its check
CATCHES = {
    "drop_key": [("keyset", 0, True, "out"), ("keyset", 1, False, "out"), ("keyset", 2, False, "out"), ("pairing4", 2, True, "out")],
    "diag_plus": [("keyset", 0, True, "out"), ("keyset", 1, True, "out"), ("keyset", 2, True, "out")],
    "diag_minus": [("keyset", 0, True, "out"), ("keyset", 1, True, "out"), ("keyset", 2, True, "out")],
    "tail_extra": [("keyset", 1, True, "out"), ("keyset", 1, False, "out"), ("keyset", 2, False, "lse")],
    "leak_next": [("keyset", 0, True, "out"), ("keyset", 0, False, "out"), ("sink", 0, True, "out")],
    "swap_s": [("pairing4", 0, True, "out"), ("pairing12", 0, True, "out"), ("pairing4", 2, False, "out"), ("pairing12", 1, True, "out")],
    "rescale_skipped": [("stair6", 0, True, "out"), ("stair20", 2, False, "out"), ("pairing12", 2, False, "out"), ("peaked8", 0, False, "out")],
    "rescale_l_only": [("stair6", 0, False, "out"), ("stair20", 2, True, "out"), ("pairing12", 0, True, "out")],
    "comb_weight_one": [("split3", 0, True, "out"), ("split136", 2, False, "out"), ("split3", 2, True, "lse"), ("sink", 2, False, "out")],
    "round_p_before_sum": [("pbias", 0, True, "lse"), ("pbias", 1, False, "lse"), ("pbias", 2, False, "lse")],
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_fails_its_designed_family(mutant):
    assert set(CATCHES) == set(R.MUTANTS)
    nq, nkv, D = R.HEADS[0]
    for fam, si, causal, which in CATCHES[mutant]:
        ql, cl = R.SHAPES[si]
        P = R.build(fam, ql, cl, nq, nkv, D, causal)
        rp = R.attn_ref(P)
        splits = 3 if mutant == "comb_weight_one" else 1
        good, good_lse = R.emulate(P, splits=splits)
        out, lse = R.emulate(P, splits=splits, mutant=mutant)
        r = _ratio(P, rp, out) if which == "out" else R.lse_ratio(lse, rp)[0]
        r0 = _ratio(P, rp, good) if which == "out" else R.lse_ratio(good_lse, rp)[0]
        print(f"{mutant:18s} on {fam:10s} shape {si} causal {causal}: {which} err / bound = {r:.2f} (unmutated {r0:.3f})")
        assert r0 <= 1.0
        assert r > 1.0, f"{mutant} must fail the {which} check on {fam} (shape {si}, causal {causal}): err / bound = {r:.3f}"


def test_what_random_data_misses():
    """randn inputs (the only ones the suite had) pass three of the mutants outright; the designed family next to each one fails it."""
    ql, cl = R.SHAPES[2]
    nq, nkv, D = R.HEADS[0]
    P = R.build("peaked4", ql, cl, nq, nkv, D, False)
    P.q = (P.q.float() / 4).to(BF16)                       # plain randn
    rp = R.attn_ref(P)
    for mutant in ("rescale_skipped", "rescale_l_only", "round_p_before_sum"):
        out, _ = R.emulate(P, mutant=mutant)
        r = R.attn_ratio(out, rp)[0]
        print(f"randn, {mutant}: err / bound = {r:.3f}")
        assert r <= 1.0
    # one dropped key in randn data: a matter of luck at 463 keys, invisible at the product's 4098
    for n, causal_ctx in ((330, 133), (4098, 0)):
        worst = []
        for seed in range(8):
            Pn = R.build("peaked4", [n], [causal_ctx], 1, 1, D, False, seed=seed)
            Pn.q = (Pn.q.float() / 4).to(BF16)
            worst.append(R.attn_ratio(R.emulate(Pn, mutant="drop_key")[0], R.attn_ref(Pn))[0])
        print(f"randn, one key of {n + causal_ctx} dropped, 8 seeds: err / bound {min(worst):.2f} .. {max(worst):.2f}")
        if n == 4098:
            assert max(worst) <= 1.0
    # and the whole-tensor metric the suite used passes a dropped key that the keyset check rejects
    ql, cl = R.SHAPES[0]
    K = R.build("keyset", ql, cl, nq, nkv, D, True)
    out, _ = R.emulate(K, mutant="drop_key")
    ref = R.attn_ref(K)["ref"]
    d = (out.double() - ref)
    assert d.abs().max().item() <= 2 * 2 ** -7 * ref.abs().max().item() and d.norm().item() <= 6e-3 * ref.norm().item(), \
        "the old allowance (2 ulp of the tensor's maximum, rel_l2 6e-3) lets the dropped key through"
    assert R.keyset_ratio(out, K)[0] > 1.0


def test_half_spacing_is_2_to_the_minus_8():
    """A correctly rounded bf16 value just above a power of two is off by almost 2^-8 of the value: u = 2^-9 would reject it."""
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -20], dtype=torch.float64)
    rel = ((x.float().to(BF16).double() - x).abs() / x).item()
    assert 2.0 ** -9 < rel <= R.U
    lo, hi = R._bf16_neighbours(torch.tensor([1.0 / 3.0, 0.5, 0.0, 5.0 / 463.0], dtype=torch.float64))
    assert (lo <= torch.tensor([1 / 3, 0.5, 0.0, 5 / 463])).all() and (hi >= torch.tensor([1 / 3, 0.5, 0.0, 5 / 463])).all()
    assert lo[1] == hi[1] == 0.5 and lo[2] == hi[2] == 0.0
    assert ((hi - lo)[[0, 3]] > 0).all() and ((hi - lo) / hi.clamp_min(1e-30) <= 2.0 ** -7).all()


def test_designed_inputs_have_their_properties():
    for (ql, cl) in R.SHAPES:
        for (nq, nkv, D) in R.HEADS:
            K = R.build("keyset", ql, cl, nq, nkv, D, False)
            cnt, n = R.keyset_counts(K)
            # a count is at most ceil(463 / D): 4 at D = 128, 8 at D = 64 -- one key moves it by 1/8 at least, 32 bf16 spacings
            assert cnt.max().item() <= (4 if D == 128 else 8) and torch.equal(cnt.sum(-1), n[:, None].expand(-1, nq))
            out, lse = R.emulate(K)
            assert torch.equal(lse.double(), torch.log2(n)[:, None].expand(-1, nq).float().double())  # every p is exactly 1
            # staircase: the row maximum really climbs by the step per tile; split136: the halves differ by > 126 log2 units
            for fam, lo in (("stair6", 4.0), ("stair20", 18.0), ("split136", 126.0)):
                P = R.build(fam, ql, cl, nq, nkv, D, False)
                if sum((c + 63) // 64 + (q + 63) // 64 for q, c in zip(ql[:1], cl[:1])) < 2:
                    continue
                q, Kk, _, C = P.sample(0, torch.float64)
                z = torch.einsum("ihd,jhd->ihj", q, Kk) * P.scale * R.LOG2E
                n0 = z.shape[-1]
                first, last = z[..., :min(64, C) if C else 64].max(-1).values, z[..., n0 - (ql[0] % 64 or 64):].max(-1).values
                gap = (first - last).abs().min().item()
                assert gap > lo, (fam, gap)
    assert 2.0 <= R._pbias_beta() ** 2 <= 7.0
