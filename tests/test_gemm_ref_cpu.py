"""The reference, bounds, designed families and schedule emulation of tests/test_gemm_designed_gpu.py, validated without a GPU
(tests/util_gemm_ref.py).

An fp32 restatement of the GEMM schedule (64-deep k-tiles, zeroed K tail, K parts + fp32 reduce, the epilogue's rounding sequence) must
reproduce the exact families bit for bit and stay inside the per-element bound on the real-valued ones; restatements that are wrong in
the ways the families are designed for must fail, and WHICH family catches WHICH mutant is asserted (``CATCHES``).

What the whole-tensor tolerance of tests/test_ops_gpu.py (``close``) cannot see on randn data is recorded in
``test_what_the_whole_tensor_tolerance_misses``: five wrong kernels pass it.
"""
import pytest
import torch

from tests import util_gemm_ref as R

BF16 = torch.bfloat16
SHAPES = [(70, 96, 72), (150, 160, 704)]          # one k-tile + a tail; 11 k-tiles (parts of 5 / 6 and 2 / 3 / 3 / 3)
SPLITS = (1, 2, 4)


@pytest.mark.parametrize("family", R.EXACT_FAMILIES)
@pytest.mark.parametrize("epi", R.EPILOGUES)
def test_emulation_is_bit_equal_on_the_exact_families(family, epi):
    for M, N, K in SHAPES:
        case = R.build(family, M, N, K, epi)
        ref = R.reference(case)
        outs = [R.emulate(case, split=s) for s in SPLITS]
        for s, out in zip(SPLITS, outs):
            R.assert_case(case, out, ref, what=f"emulation split {s}")
        if case.epi == R.EPI_NONE:
            assert all(torch.equal(R.bits(outs[0]), R.bits(o)) for o in outs[1:]), "split and unsplit schedules must agree bit for bit"


@pytest.mark.parametrize("family", ["scaled", "cancel", "edges"])
@pytest.mark.parametrize("epi", R.EPILOGUES)
def test_emulation_and_fp32_matmul_stay_within_the_bound(family, epi):
    for M, N, K in [(70, 96, 80), (150, 160, 704)]:
        case = R.build(family, M, N, K, epi)
        ref = R.reference(case)
        res = {f"split{s}": R.assert_case(case, R.emulate(case, split=s), ref, what=f"emulation split {s}") for s in SPLITS}
        res["matmul"] = R.assert_case(case, R.matmul32(case), ref, what="fp32 matmul")
        print(f"{case.name}: err / bound " + " ".join(f"{k} {v:.3f}" for k, v in res.items()))


def test_fp32_matmul_on_randn_stays_within_the_bound():
    """The bound is not fitted to the families: plain randn operands through torch's fp32 matmul (worst err / bound ~0.75: the output
    rounding alone reaches u / (1 + u) |t| on an element just above a power of two)."""
    g = torch.Generator().manual_seed(0)
    M, N, K = 300, 264, 1152
    A, W = torch.randn(M, K, generator=g).to(BF16), (torch.randn(N, K, generator=g) * K ** -0.5).to(BF16)
    b, Rr = (torch.randn(N, generator=g) * 0.1).to(BF16), torch.randn(M, N, generator=g).to(BF16)
    for res in (False, True):
        C0 = Rr.clone() if res else torch.full((M, N), float("nan"), dtype=BF16)
        case = R.Case("randn", A, [dict(W=W, bias=b, a_rows=None, c_rows=None, M=M)], res=res, C0=C0)
        q = R.assert_case(case, R.matmul32(case), what="fp32 matmul")
        print(f"randn {M}x{N}x{K} residual {res}: err / bound = {q:.3f}")
        assert q > 0.3, "a bound this far above an honest kernel's error could not reject a misplaced rounding"


# mutant -> [(family, epilogue, K parts)]: every listed case must FAIL its check (and the honest emulation pass it)
CATCHES = {
    "drop_chunk_ktile": [("kprobe", "plain", 1), ("exact", "bias", 1), ("exact", "groups", 1)],
    "double_chunk_ktile": [("kprobe", "plain", 1), ("exact", "res", 1)],
    "drop_chunk_ksplit": [("kprobe", "plain", 2), ("kprobe", "bias_res", 4), ("exact", "plain", 2)],
    "double_chunk_ksplit": [("kprobe", "plain", 2), ("exact", "res", 4)],
    "parts_off_by_one": [("exact", "plain", 2), ("kprobe", "bias", 4), ("roundpoint", "plain", 2)],
    "ktail_not_zeroed": [("exact", "plain", 1), ("kprobe", "bias", 1)],
    "partials_bf16": [("roundpoint", "plain", 2), ("roundpoint", "bias_res", 4)],
    "bias_after_rounding": [("roundpoint", "bias", 1), ("roundpoint", "bias_res", 2), ("roundpoint", "groups", 1)],
    "merged_residual": [("roundpoint", "res", 1), ("roundpoint", "bias_res", 2), ("roundpoint", "groups", 1)],
    "gelu_unrounded": [("roundpoint", "bias_gelu", 1), ("roundpoint", "silu", 1)],
    "clamp_dup": [("edges", "plain", 1), ("edges", "groups", 1), ("edges", "gather", 1)],
    "bias_chunk_prev": [("exact", "bias", 1), ("exact", "bias_res", 2), ("scaled", "bias", 1)],
    "swiglu_swap": [("exact", "swiglu", 1), ("scaled", "swiglu", 1), ("roundpoint", "swiglu", 1)],
    "wrong_group_weight": [("exact", "groups", 1), ("scaled", "groups", 2), ("kprobe", "groups", 1)],
    "crows_off_by_one": [("exact", "groups", 1), ("edges", "groups", 1), ("edges", "gather", 1)],
    "stale_lds_chunk": [("exact", "plain", 1), ("exact", "groups", 2), ("scaled", "plain", 1)],
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_caught_by_its_families(mutant):
    assert set(CATCHES) == set(R.MUTANTS)
    for family, epi, split in CATCHES[mutant]:
        M, N, K = (150, 160, 712) if mutant == "ktail_not_zeroed" else (150, 160, 704)
        case = R.build(family, M, N, K, epi)
        ref = R.reference(case)
        R.assert_case(case, R.emulate(case, split=split), ref, what="honest emulation")
        assert not R.passes(case, R.emulate(case, split=split, mutant=mutant), ref), f"{mutant} passes {family}/{epi} with {split} K parts"


def test_a_merged_rounding_needs_the_membership_check():
    """bf16(t + r) lies inside the stated two-rounding bound on real-valued data (it is the more accurate result): only the set of
    legitimate two-rounding results rejects it."""
    case = R.build("scaled", 150, 160, 704, "bias_res")
    ref = R.reference(case)
    q, _, member = R.ratio(case, R.emulate(case, mutant="merged_residual"), ref)
    assert q <= 1.0 and member is False
    q, _, member = R.ratio(case, R.emulate(case), ref)
    assert q <= 1.0 and member is True


def test_what_the_whole_tensor_tolerance_misses():
    """Five wrong kernels on randn operands at 1100 x 264 x 1152 against ``close`` of tests/test_ops_gpu.py (max|d| <= ulps 2^-7 max|ref|,
    rel-L2 4e-3): all five PASS it.  The designed families above reject each of them."""
    from tests.test_ops_gpu import close, ref_gemm
    g = torch.Generator().manual_seed(0)
    M, N, K = 1100, 264, 1152
    A, W = torch.randn(M, K, generator=g).to(BF16), (torch.randn(N, K, generator=g) * K ** -0.5).to(BF16)
    b, Rr = (torch.randn(N, generator=g) * 0.1).to(BF16), torch.randn(M, N, generator=g).to(BF16)

    def measure(got, ref, ulps):
        close(got, ref, ulps=ulps)                                    # raises if the old check would have noticed
        d = (got.float() - ref.float()).abs()
        return d.max().item() / (ulps * 2 ** -7 * ref.float().abs().max().item()), (got.float() - ref.float()).norm().item() / ref.float().norm().item() / 4e-3

    rows = {}
    nk = K // 64
    parts = [A.float()[:, 64 * (nk * p // 4):64 * (nk * (p + 1) // 4)] @ W.float()[:, 64 * (nk * p // 4):64 * (nk * (p + 1) // 4)].t() for p in range(4)]
    acc = sum(p.to(BF16).float() for p in parts)
    rows["K-split partials rounded to bf16"] = measure((acc + b.float()).to(BF16), ref_gemm(A, W, b), 1)
    acc = A.float() @ W.float().t()
    rows["bias added after the rounding"] = measure((acc.to(BF16).float() + b.float()).to(BF16), ref_gemm(A, W, b), 1)
    rows["residual merged into one rounding"] = measure((acc + b.float() + Rr.float()).to(BF16), ref_gemm(A, W, b, 0, Rr), 2)
    As = A.clone()
    As[::16] = (A[::16].float() * 2.0 ** -8).to(BF16)
    ref = ref_gemm(As, W, b * 0)
    zero = ref.clone()
    zero[::16] = 0
    rows["small rows written as zero"] = measure(zero, ref, 1)
    half = ref.clone()
    half[::16] = (ref[::16].float() * 1.5).to(BF16)
    rows["small rows off by 50 %"] = measure(half, ref, 1)
    for k, (a, l2) in rows.items():
        print(f"{k:40s} max / allowed {a:.2f}   rel-L2 / allowed {l2:.2f}")
        assert a < 1 and l2 < 1
    # ... and the per-element bound rejects the two that need no designed input
    case = R.Case("small rows", As, [dict(W=W, bias=None, a_rows=None, c_rows=None, M=M)], C0=torch.full((M, N), float("nan"), dtype=BF16))
    assert not R.passes(case, zero) and not R.passes(case, half) and R.passes(case, ref)


def test_leftover_split_rule_at_the_claimed_shapes():
    """The host-only K-split rule (host_plan.cpp, pq_leftover_split through bagel_gemm_leftover_split) at the shapes tests/test_gemm_designed_gpu.py
    claims to cover on 8 workgroups with the 64 MB workspace: a routing change cannot silently drop the K-split coverage."""
    import ctypes
    from bagel_amd._lib import lib
    from tests.test_gemm_designed_gpu import CLAIMED_WGS8
    for (M, N, K), (nblk, n_full, s) in CLAIMED_WGS8.items():
        nf, ks = ctypes.c_int32(-1), ctypes.c_int32(-1)
        assert nblk == -(-M // 256) * -(-N // 256)
        assert lib().bagel_gemm_leftover_split(nblk, 8, K // 64, 256 * 256 * 256 * 4, 0, 0, ctypes.byref(nf), ctypes.byref(ks)) == 0
        assert (ks.value, nf.value if ks.value > 1 else nblk) == (s, n_full), ((M, N, K), nf.value, ks.value)
