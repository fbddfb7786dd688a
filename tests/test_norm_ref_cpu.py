"""CPU validation of tests/util_norm_ref.py, the module tests/test_norm_designed_gpu.py holds the norm / rotary kernels to: the honest fp32
restatement equals the one legal pattern on the exact families and stays inside the legal sets and bounds on the real-valued ones, it agrees with
oracle.bagel_oracle and tests/mock_ops.py, and every way of getting a kernel subtly wrong that the families are designed for is rejected by the
family named for it (``CATCHES``).  What the whole-tensor tolerance of tests/test_ops_gpu.py (``close``) cannot see on the existing tests' randn
inputs is recorded in ``test_what_the_whole_tensor_tolerance_misses``.
"""
import pytest
import torch

from tests import util_norm_ref as R

BF16 = torch.bfloat16
MAX_SHARE = 1.0 / 8


def _rms(family, rows=9, cols=520, **kw):
    return R.rms_case(family, rows, cols, **kw)


def _check_rms(case, got, what=""):
    return R.check(case.name, got, case.y0, case.region, R.rms_legal(case), what)


def _check_qk(case, got, what=""):
    return R.check(case.name, got, case.qkv0, case.region, R.qk_legal(case), what)


def _check_ln(case, got, what=""):
    ref = R.ln_reference(case)
    q = R.ln_ratio(case, got, ref)
    assert q <= 1.0, f"{what} {case.name}: err / bound = {q:.3f}"
    return R.check(case.name, got, case.y0, case.region, ref["legal"], what)


def _ok(fn, *a):
    try:
        fn(*a)
        return True
    except AssertionError:
        return False


# ------------------------------------------------------------------------------------------------------------
# the honest restatement
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [8, 512, 520, 3584, 4096, 4104, 8200])
@pytest.mark.parametrize("routed", [None, "mixed", "zeros", "ones"])
def test_rmsnorm_restatement_is_the_one_pattern_on_the_exact_family(cols, routed):
    case = _rms("exact", 7, cols, routed=routed, ldx=cols + 24, ldy=cols + 8)
    L = R.rms_legal(case)
    assert L.share() == 0.0
    assert _check_rms(case, R.emu_rmsnorm(case)) == 0.0
    # the value itself: w m / 2
    y = R.emu_rmsnorm(case)[:7, :cols].float()
    a = 2.0 ** (2 + torch.arange(7) % 4).float()
    assert torch.equal(y, case.xv().float() / (2 * a[:, None]) * case.weight())


@pytest.mark.parametrize("family", ["castpoint", "tiny"])
@pytest.mark.parametrize("cols", [8, 512, 3584, 4104, 8200])
def test_rmsnorm_restatement_inside_the_legal_sets(family, cols):
    case = _rms(family, 9, cols, routed="mixed")
    share = _check_rms(case, R.emu_rmsnorm(case))
    print(f"{case.name}: ambiguous share {share:.4f}")
    assert share <= MAX_SHARE


@pytest.mark.parametrize("gen", [0, 1])
@pytest.mark.parametrize("hd,dp,nq,nkv", [(128, 128, 28, 4), (64, 64, 3, 3), (32, 64, 5, 2)])
def test_qknorm_restatement_on_every_family(hd, dp, nq, nkv, gen):
    for family in ("exact", "tables", "castpoint", "tiny"):
        for use_norm in (0, 1):
            if family == "exact" and not use_norm:
                continue
            case = R.qk_case(family, 7, nq, nkv, hd, dp, gen, use_norm, routed="mixed" if gen else None)
            share = _check_qk(case, R.emu_qknorm(case))
            print(f"{case.name}: ambiguous share {share:.4f}")
            assert share <= MAX_SHARE and (share == 0.0 or (use_norm and family not in ("exact",)))
            if not use_norm:
                assert R.qk_legal(case).share() == 0.0


@pytest.mark.parametrize("family", ["pivot", "tiny", "benign"])
@pytest.mark.parametrize("cols", [8, 72, 1152, 4104])
def test_layernorm_restatement_inside_bound_and_interval(family, cols):
    case = R.ln_case(family, 7, cols)
    ref = R.ln_reference(case)
    share = _check_ln(case, R.emu_layernorm(case))
    q = R.ln_ratio(case, R.emu_layernorm(case), ref)
    print(f"{case.name}: err / bound {q:.3f}, ambiguous share {share:.4f}")
    assert bool(torch.isfinite(ref["bound"]).all())
    assert share <= MAX_SHARE
    if family == "pivot":                       # tight where |x| >> |x - mean|: the carried errors stay far below the output rounding
        assert float((ref["E"] / (R.U * ref["t"].abs()).clamp_min(1e-30))[ref["t"].abs() > 0.05].max()) < 0.25


POSITIONS = [0, 1, 2, 63, 64, 65, 127, 128, 1023, 1024, 4095, 4096, 4097, 4097, 16384, 31999, 32000, 32000, 32767]


@pytest.mark.parametrize("half,theta", [(16, 1e6), (36, 1e4), (64, 1e6)])
def test_rope_table_restatement_inside_the_intervals(half, theta):
    pos = torch.tensor(POSITIONS, dtype=torch.long)
    inv = R.inv_freq(2 * half, theta)
    Lc, Ls = R.rope_table_legal(pos, inv)
    c, s = R.emu_rope_table(pos, inv)
    assert bool(Lc.ok(c).all()) and bool(Ls.ok(s).all())
    print(f"rope_table half {half}: ambiguous share cos {Lc.share():.4f} sin {Ls.share():.4f}")
    assert max(Lc.share(), Ls.share()) <= MAX_SHARE


@pytest.mark.parametrize("kind", ["tables", "oracle"])
@pytest.mark.parametrize("hd,dp", [(72, 72), (64, 64), (16, 32), (72, 80)])
def test_rope2d_restatement_equals_the_mock(kind, hd, dp):
    from tests import mock_ops
    case = R.Rope2dCase(kind, 9, 6, hd, dp)
    buf, _ = R.emu_rope2d(case)
    ref = mock_ops.rope2d(case.qkv0.clone()[:case.rows], case.tables, case.pos_ids, case.nheads, hd, dp)
    assert torch.equal(R.bits(buf[:case.rows]), R.bits(ref))
    assert bool((R.bits(buf) == R.bits(case.qkv0))[~case.region].all())


# ------------------------------------------------------------------------------------------------------------
# oracle and mock
# ------------------------------------------------------------------------------------------------------------
def test_agrees_with_the_oracle_and_the_mock_on_benign_inputs():
    from oracle import bagel_oracle as O
    from tests import mock_ops
    # rmsnorm
    case = _rms("castpoint", 9, 512, routed=None)
    y = R.emu_rmsnorm(case)[:9, :512]
    o = O.rmsnorm(case.xv(), case.w0, 1e-6)
    assert float((R.bits(y) != R.bits(o.to(BF16))).float().mean()) < 0.01      # torch.mean and the chunked sum may differ in inv by an ulp
    m = mock_ops.rmsnorm(case.xv(), case.w0, torch.empty(9, 512, dtype=BF16), 1e-6)
    assert float((R.bits(y) != R.bits(m)).float().mean()) < 0.01
    assert bool(R.rms_legal(case).ok(m).all()) and bool(R.rms_legal(case).ok(o.to(BF16)).all())
    # layernorm
    lc = R.ln_case("benign", 9, 1152)
    m = mock_ops.layernorm(lc.xv(), lc.w0, lc.bias, torch.empty(9, 1152, dtype=BF16), 1e-6)
    assert bool(R.ln_reference(lc)["legal"].ok(m).all())
    # rope tables
    pos = torch.tensor(POSITIONS, dtype=torch.long)
    for hd in (32, 128):
        c, s = R.emu_rope_table(pos, R.inv_freq(hd))
        oc, os_ = O.rope_tables(pos, hd, 1e6, BF16)
        assert torch.equal(R.bits(c), R.bits(oc[:, :hd // 2])) and torch.equal(R.bits(s), R.bits(os_[:, :hd // 2]))
        mc, ms = mock_ops.rope_table(pos, R.inv_freq(hd))
        assert torch.equal(R.bits(c), R.bits(mc)) and torch.equal(R.bits(s), R.bits(ms))
    # qknorm + rope against apply_rope of the oracle (und: bf16 tensors; gen: fp32 then one rounding) and against the mock, every mode
    for gen in (0, 1):
        for use_norm in (0, 1):
            qc = R.qk_case("castpoint", 9, 4, 2, 128, 128, gen, use_norm, routed=None)
            got = R.emu_qknorm(qc)
            mk = mock_ops.qknorm_rope(qc.qkv0.clone()[:9], qc.cos, qc.sin, qc.w[0], qc.w[1], None, None, None, 4, 2, 128, 128, 1e-6, gen, use_norm)
            assert bool(R.qk_legal(qc).ok(qc.heads(mk)).all())
            x = qc.heads()
            cos, sin = torch.cat([qc.cos, qc.cos], -1), torch.cat([qc.sin, qc.sin], -1)
            if gen:
                xf = x.float()
                if use_norm:
                    xf = torch.cat([O.rmsnorm(xf[:, :4], qc.w[0], 1e-6), O.rmsnorm(xf[:, 4:], qc.w[1], 1e-6)], 1)
                rq, _ = O.apply_rope(xf, xf, cos.float(), sin.float())
            else:
                xn = torch.cat([O.rmsnorm(x[:, :4], qc.w[0], 1e-6), O.rmsnorm(x[:, 4:], qc.w[1], 1e-6)], 1) if use_norm else x
                rq, _ = O.apply_rope(xn, xn, cos, sin)
            assert bool(R.qk_legal(qc).ok(rq.to(BF16)).all()), (gen, use_norm)
    # rope2d tables of the oracle's construction at the SigLIP head dim
    ch, sh, cw, sw = O.rope2d_tables(36, 4, 4)
    case = R.Rope2dCase("oracle", 9, 6, 72, 72)
    assert case.tables[0].shape[1] == ch.shape[1] == 36
    assert torch.equal(R.bits(case.tables[2][:4]), R.bits(cw[:4].to(BF16)))     # column axis: positions 0 .. 3 of the first grid row


# ------------------------------------------------------------------------------------------------------------
# the cast points
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_norm", [0, 1])
def test_castpoint_und_and_gen_reject_each_other(use_norm):
    shares = []
    for gen in (0, 1):
        case = R.qk_case("castpoint", 9, 5, 2, 128, 128, gen, use_norm)
        honest, other = R.emu_qknorm(case), R.emu_qknorm(case, "und_in_gen" if gen else "gen_in_und")
        _check_qk(case, honest)
        assert not _ok(_check_qk, case, other)
        shares.append(float((R.bits(honest) != R.bits(other))[case.region].float().mean()))
    print(f"und / gen differ on {shares[0]:.3f} of the elements (use_norm = {use_norm})")
    assert min(shares) >= 0.25


def test_castpoint_merged_rounding_differs_on_a_fifth():
    for cols in (512, 3584):
        case = _rms("castpoint", 9, cols)
        d = float((R.bits(R.emu_rmsnorm(case)) != R.bits(R.emu_rmsnorm(case, "merged_rounding")))[case.region].float().mean())
        print(f"merged rounding differs on {d:.3f} at {cols} columns")
        assert d >= 0.2


def test_tiny_rows_need_eps():
    case = _rms("tiny", 8, 512)
    d = (R.bits(R.emu_rmsnorm(case)) != R.bits(R.emu_rmsnorm(case, "eps_dropped")))[:8, :512].float().mean(1)
    small = torch.arange(8) % 4 != 1
    print(f"dropping eps changes {d.tolist()} of each row")
    assert float(d[small].min()) >= 0.9 and float(d[~small].max()) <= 0.05


def test_pivot_family_rejects_the_one_pass_variance():
    """The one-pass fp32 variance E[x^2] - E[x]^2 at a pivot of 362 sigma.  At 8 columns every sum of the 8-bit inputs is exact in fp32 either
    way, so the family can reject it from 72 columns on."""
    for cols in (72, 1152, 4104):
        case = R.ln_case("pivot", 8, cols)
        _check_ln(case, R.emu_layernorm(case))
        assert not _ok(_check_ln, case, R.emu_layernorm(case, "one_pass_variance")), cols
    x = R.fam_pivot(4, 1152).double()
    assert float((x.mean(1).abs() / x.var(1, unbiased=False).sqrt()).min()) > 300


# ------------------------------------------------------------------------------------------------------------
# mutants: which family rejects which wrong restatement
# ------------------------------------------------------------------------------------------------------------
def _qk(family, gen, use_norm=1, hd=128, dp=128, nq=5, nkv=2, routed=None, rows=7):
    return ("qk", lambda: R.qk_case(family, rows, nq, nkv, hd, dp, gen, use_norm, routed=routed))


CATCHES = {
    # rmsnorm
    "rms:merged_rounding": [("rms", lambda: _rms("castpoint", 9, 512)), ("rms", lambda: _rms("castpoint", 9, 4104))],
    "rms:eps_dropped": [("rms", lambda: _rms("tiny", 9, 512)), ("rms", lambda: _rms("tiny", 9, 4104))],
    "rms:eps_after_rsqrt": [("rms", lambda: _rms("tiny", 9, 512))],
    "rms:divisor_ld": [("rms", lambda: _rms("exact", 9, 8, ldx=16)), ("rms", lambda: _rms("exact", 9, 512, ldx=1024)), ("rms", lambda: _rms("castpoint", 9, 4104))],
    "rms:wrong_expert": [("rms", lambda: _rms("exact", 9, 520, routed="mixed")), ("rms", lambda: _rms("exact", 9, 4104, routed="ones"))],
    "rms:tail_chunk_dropped": [("rms", lambda: _rms("exact", 9, 520)), ("rms", lambda: _rms("castpoint", 9, 4104)), ("rms", lambda: _rms("castpoint", 9, 8200))],
    # layernorm
    "ln:one_pass_variance": [("ln", lambda: R.ln_case("pivot", 7, 72)), ("ln", lambda: R.ln_case("pivot", 7, 1152)), ("ln", lambda: R.ln_case("pivot", 7, 4104))],
    "ln:unbiased_variance": [("ln", lambda: R.ln_case("pivot", 7, 8)), ("ln", lambda: R.ln_case("benign", 7, 72))],
    "ln:bias_after_rounding": [("ln", lambda: R.ln_case("benign", 7, 72)), ("ln", lambda: R.ln_case("benign", 7, 1152))],
    "ln:eps_dropped": [("ln", lambda: R.ln_case("tiny", 7, 72)), ("ln", lambda: R.ln_case("tiny", 7, 1152))],
    # qknorm_rope
    "qk:und_in_gen": [_qk("castpoint", 1), _qk("castpoint", 1, use_norm=0), _qk("tables", 1, use_norm=0)],
    "qk:gen_in_und": [_qk("castpoint", 0), _qk("castpoint", 0, use_norm=0), _qk("tables", 0, use_norm=0)],
    "qk:divisor_dp": [_qk("exact", 0, hd=32, dp=64), _qk("exact", 1, hd=32, dp=64)],
    "qk:rotate_sign": [_qk("exact", 0), _qk("tables", 1, use_norm=0), _qk("tables", 0, use_norm=0, hd=32, dp=64)],
    "qk:cos_not_wrapped": [_qk("tables", 0, use_norm=0), _qk("tables", 1, use_norm=0, hd=64, dp=64), _qk("exact", 0)],
    "qk:table_row_shift": [_qk("tables", 0, use_norm=0), _qk("exact", 1)],
    "qk:k_uses_q_weight": [_qk("exact", 0), _qk("exact", 1, routed="mixed")],
    "qk:expert_ignored": [_qk("exact", 1, routed="mixed"), _qk("exact", 1, routed="ones")],
    "qk:v_written": [_qk("exact", 0), _qk("tables", 1, use_norm=0)],
    "qk:pad_written": [_qk("exact", 0, hd=32, dp=64), _qk("tables", 1, use_norm=0, hd=32, dp=64)],
    # rope2d
    "rope2d:hw_swapped": [("rope2d", lambda: R.Rope2dCase("tables", 9, 6, 72, 72)), ("rope2d", lambda: R.Rope2dCase("oracle", 9, 6, 72, 72))],
    "rope2d:partner_h2": [("rope2d", lambda: R.Rope2dCase("tables", 9, 6, 72, 80)), ("rope2d", lambda: R.Rope2dCase("tables", 9, 6, 16, 16))],
    "rope2d:pos_ignored": [("rope2d", lambda: R.Rope2dCase("tables", 9, 6, 64, 64)), ("rope2d", lambda: R.Rope2dCase("oracle", 9, 6, 72, 72))],
    "rope2d:k_skipped": [("rope2d", lambda: R.Rope2dCase("tables", 9, 6, 72, 72))],
    # rope_table
    "rope_table:angle_in_float64": [("rope_table", lambda: (torch.tensor(POSITIONS, dtype=torch.long), R.inv_freq(128)))],
    # decode_qkv_post
    "decode:pad_not_zeroed": [("decode", lambda: R.DecodeCase("exact", 3, 1, 32, 64, 1))],
    "decode:slot_off_by_one": [("decode", lambda: R.DecodeCase("exact", 28, 4, 128, 128, 1))],
    "decode:page_boundary": [("decode", lambda: R.DecodeCase("tables", 12, 2, 64, 64, 0))],
    "decode:head_tail_dropped": [("decode", lambda: R.DecodeCase("exact", 28, 4, 128, 128, 1)), ("decode", lambda: R.DecodeCase("tables", 3, 1, 128, 128, 0))],
    "decode:v_roped": [("decode", lambda: R.DecodeCase("exact", 12, 2, 64, 64, 1))],
}


def _verdicts(kind, case, mutant):
    """-> (the honest restatement passes, the mutant passes)."""
    if kind == "rms":
        return _ok(_check_rms, case, R.emu_rmsnorm(case)), _ok(_check_rms, case, R.emu_rmsnorm(case, mutant))
    if kind == "ln":
        return _ok(_check_ln, case, R.emu_layernorm(case)), _ok(_check_ln, case, R.emu_layernorm(case, mutant))
    if kind == "qk":
        return _ok(_check_qk, case, R.emu_qknorm(case)), _ok(_check_qk, case, R.emu_qknorm(case, mutant))
    if kind == "rope2d":
        want, _ = R.emu_rope2d(case)
        return True, torch.equal(R.bits(R.emu_rope2d(case, mutant)[0]), R.bits(want))
    if kind == "rope_table":
        pos, inv = case
        Lc, Ls = R.rope_table_legal(pos, inv)
        h, m = R.emu_rope_table(pos, inv), R.emu_rope_table(pos, inv, mutant)
        return bool(Lc.ok(h[0]).all() and Ls.ok(h[1]).all()), bool(Lc.ok(m[0]).all() and Ls.ok(m[1]).all())
    assert kind == "decode"
    return R.decode_passes(case, R.emu_decode(case)), R.decode_passes(case, R.emu_decode(case, mutant))


@pytest.mark.parametrize("mutant", sorted(CATCHES))
def test_every_mutant_is_rejected_by_its_family(mutant):
    every = [f"rms:{m}" for m in R.RMS_MUTANTS] + [f"ln:{m}" for m in R.LN_MUTANTS] + [f"qk:{m}" for m in R.QK_MUTANTS] + \
        [f"rope2d:{m}" for m in R.ROPE2D_MUTANTS] + [f"rope_table:{m}" for m in R.ROPE_TABLE_MUTANTS] + [f"decode:{m}" for m in R.DECODE_MUTANTS]
    assert set(CATCHES) == set(every)
    for kind, make in CATCHES[mutant]:
        case = make()
        honest, wrong = _verdicts(kind, case, mutant.split(":")[1])
        name = getattr(case, "name", kind)
        assert honest, f"the honest restatement fails {name}"
        assert not wrong, f"{mutant} passes {name}"


@pytest.mark.parametrize("nq,nkv,hd,dp,use_norm", [(28, 4, 128, 128, 1), (3, 1, 32, 64, 1), (12, 2, 64, 64, 0), (3, 1, 128, 128, 1)])
def test_decode_restatement_on_every_family(nq, nkv, hd, dp, use_norm):
    for family in ("exact", "tables", "castpoint", "tiny"):
        if family == "exact" and not use_norm:
            continue
        dc = R.DecodeCase(family, nq, nkv, hd, dp, use_norm)
        share = R.check_decode(dc, R.emu_decode(dc))
        assert share <= MAX_SHARE and (use_norm or share == 0.0)
        # slots: first of a page, last of a page, first of the second page, last of the second page
        assert (dc.kv_len % 64).tolist() == [0, 63, 0, 63]


def test_empty_problems():
    for case in (_rms("exact", 0, 512), _rms("castpoint", 0, 8)):
        assert torch.equal(R.bits(R.emu_rmsnorm(case)), R.bits(case.y0))
    lc = R.ln_case("benign", 0, 72)
    assert torch.equal(R.bits(R.emu_layernorm(lc)), R.bits(lc.y0))
    qc = R.qk_case("tables", 0, 4, 1, 64, 64, 0, 0)
    assert torch.equal(R.bits(R.emu_qknorm(qc)), R.bits(qc.qkv0))


# ------------------------------------------------------------------------------------------------------------
# what ``close`` cannot see
# ------------------------------------------------------------------------------------------------------------
def test_what_the_whole_tensor_tolerance_misses():
    """Wrong restatements on the randn inputs of tests/test_ops_gpu.py (test_rmsnorm_and_expert_routing, test_layernorm, test_qknorm_rope)
    against ``close`` (max|d| <= 2^-7 max|ref|, rel-L2 4e-3): every one listed in ``MISSED`` PASSES it.  The families above reject each of them."""
    from tests.test_ops_gpu import close
    missed = []

    def accepted(got, ref):
        try:
            close(got, ref)
            return True
        except AssertionError:
            return False

    # rmsnorm: x = 3 randn, w = 1 + 0.1 randn, 37 x 3584 unpadded
    g = torch.Generator().manual_seed(1)
    rows, cols = 37, 3584
    case = R.RowCase("randn", (torch.randn(rows, cols, generator=g) * 3).to(BF16), R.real_weight(cols, 2), R.real_weight(cols, 3),
                     (torch.arange(rows) % 3 == 1).to(torch.int32), cols, cols, 1e-6)
    ref = R.emu_rmsnorm(case)[:rows]
    for m in ("merged_rounding", "eps_dropped", "eps_after_rsqrt", "tail_chunk_dropped"):
        if accepted(R.emu_rmsnorm(case, m)[:rows], ref):
            missed.append("rms:" + m)
    # layernorm: zero-mean rows 257 x 1152
    lc = R.RowCase("randn", (torch.randn(257, 1152, generator=g) * 2).to(BF16), R.real_weight(1152, 2), None, None, 1152, 1152, 1e-6,
                   bias=(0.1 * torch.randn(1152, generator=g)).to(BF16))
    ref = R.emu_layernorm(lc)[:257]
    for m in R.LN_MUTANTS:
        if accepted(R.emu_layernorm(lc, m)[:257], ref):
            missed.append("ln:" + m)
    # qknorm_rope: the castpoint case is the existing test's input distribution (randn heads, oracle tables)
    for gen in (0, 1):
        qc = R.qk_case("castpoint", 37, 28, 4, 128, 128, gen, 1)
        ref = qc.heads(R.emu_qknorm(qc))
        m = "und_in_gen" if gen else "gen_in_und"
        if accepted(qc.heads(R.emu_qknorm(qc, m)), ref):
            missed.append("qk:" + m)
    print("close accepts:", missed)
    MISSED = ["rms:merged_rounding", "rms:eps_dropped", "rms:eps_after_rsqrt", "rms:tail_chunk_dropped", "ln:one_pass_variance", "ln:unbiased_variance",
              "ln:bias_after_rounding", "ln:eps_dropped", "qk:gen_in_und", "qk:und_in_gen"]
    assert missed == MISSED
