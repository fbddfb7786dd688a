"""The norm and rotary kernels (norm.hip: rmsnorm, rmsnorm_fp8, layernorm, rope_table, qknorm_rope, rope2d; decode.hip: decode_qkv_post) on the
designed inputs of tests/util_norm_ref.py.  Exact, designed-table, no-norm and rope2d cases: the one legal bit pattern.  Real-valued cases: inside
the legal sets / the float64 bound, with at most 1/8 of the elements having more than one legal pattern.  Every output buffer is larger than the
problem and pre-filled with a sentinel; whatever must not be written is compared bit for bit.

Every test prints its ambiguous share (and, for layernorm, its worst err / bound) per case."""
import pytest
import torch

from tests import util_norm_ref as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda"
MAX_SHARE = 1.0 / 8
RMS_COLS = [8, 512, 520, 3584, 4096, 4104, 8200]       # 4096 / 4104: the two sides of the register / streaming switch (nch <= 512)


def ops():
    from bagel_amd import ops as o
    return o


def _report(case, share, extra=""):
    print(f"{case.name}: ambiguous share {share:.4f}{extra}")
    assert share <= MAX_SHARE, f"{case.name}: {share:.3f} of the elements have more than one legal pattern"
    if case.exact:
        assert share == 0.0


# ------------------------------------------------------------------------------------------------------------
# rmsnorm
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["exact", "castpoint", "tiny"])
@pytest.mark.parametrize("cols", RMS_COLS)
def test_rmsnorm(cols, family):
    """Strided x and y with different leading dimensions (NaN past the columns of x, sentinels around y), rows = 1, 2, 3 mod 4."""
    for routed, rows in ((None, 9), ("mixed", 7), ("zeros", 6), ("ones", 5)):
        case = R.rms_case(family, rows, cols, ldx=cols + 8, ldy=cols + 24, routed=routed)
        got = R.run_rmsnorm(ops(), case)
        _report(case, R.check(case.name, got, case.y0, case.region, R.rms_legal(case)))


def test_rmsnorm_no_rows():
    case = R.rms_case("exact", 0, 512)
    assert torch.equal(R.bits(R.run_rmsnorm(ops(), case)), R.bits(case.y0))


@pytest.mark.parametrize("cols", [512, 4096, 4104])
def test_rmsnorm_fp8_equals_rmsnorm_then_the_quantiser(cols):
    """Codes and scales bit-equal to the GPU rmsnorm (itself held to the legal sets above) followed by oracle/fp8.py's quantiser, on strided x and q;
    nothing outside the [rows, cols] block of q or past the rows of the scales is written."""
    from oracle import fp8 as F8
    o = ops()
    rows = 7
    for family in ("castpoint", "tiny", "exact"):
        case = R.rms_case(family, rows, cols, ldx=cols + 8, ldy=cols + 24)
        y = R.run_rmsnorm(o, case)
        R.check(case.name, y, case.y0, case.region, R.rms_legal(case))
        qr, sr = F8.quantize_rows_fp8(y[:rows, :cols].contiguous())
        q = torch.full((rows + 1, cols + 16), 0xAB, dtype=torch.uint8, device=DEV)
        s = torch.full((rows + 1,), -7.0, dtype=torch.float32, device=DEV)
        o.rmsnorm_fp8(case.x.to(DEV)[:, :cols], case.w0.to(DEV), q[:rows, :cols], s[:rows], case.eps)
        q, s = q.cpu(), s.cpu()
        assert torch.equal(s[:rows], sr), f"{case.name}: scales differ"
        bad = q[:rows, :cols] != qr
        assert not bool(bad.any()), f"{case.name}: {int(bad.sum())} codes differ, first at {bad.nonzero()[0].tolist()}"
        assert bool((q[:rows, cols:] == 0xAB).all()) and bool((q[rows:] == 0xAB).all()) and float(s[rows]) == -7.0, f"{case.name}: wrote outside the result"
        print(f"{case.name}: fp8 codes and scales bit-equal")


# ------------------------------------------------------------------------------------------------------------
# layernorm
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["pivot", "tiny", "benign"])
@pytest.mark.parametrize("cols", [8, 72, 1152, 4104])
def test_layernorm(cols, family):
    for rows in (7, 6, 5):
        case = R.ln_case(family, rows, cols, ldx=cols + 8, ldy=cols + 24)
        ref = R.ln_reference(case)
        got = R.run_layernorm(ops(), case)
        q = R.ln_ratio(case, got, ref)
        print(f"{case.name}: err / bound {q:.3f}")
        assert q <= 1.0, f"{case.name}: err / bound = {q:.3f}"
        _report(case, R.check(case.name, got, case.y0, case.region, ref["legal"]))


def test_layernorm_no_rows():
    case = R.ln_case("benign", 0, 72)
    assert torch.equal(R.bits(R.run_layernorm(ops(), case)), R.bits(case.y0))


# ------------------------------------------------------------------------------------------------------------
# rope_table
# ------------------------------------------------------------------------------------------------------------
# 0, 1, the page (64) and power-of-two edges, the model's largest positions, repeats
POSITIONS = [0, 1, 2, 63, 64, 65, 127, 128, 1023, 1024, 4095, 4096, 4097, 4097, 16384, 31999, 32000, 32000, 32767, 0]


@pytest.mark.parametrize("half,theta", [(16, 1e6), (36, 1e4), (64, 1e6)])
def test_rope_table(half, theta):
    pos = torch.tensor(POSITIONS, dtype=torch.long)
    inv = R.inv_freq(2 * half, theta)
    Lc, Ls = R.rope_table_legal(pos, inv)
    cos, sin = ops().rope_table(pos.to(DEV), inv.to(DEV))
    cos, sin = cos.cpu(), sin.cpu()
    for name, got, L in (("cos", cos, Lc), ("sin", sin, Ls)):
        ok = L.ok(got)
        if not bool(ok.all()):
            r, c = (~ok).nonzero()[0].tolist()
            raise AssertionError(f"rope_table {name} half {half}: {int((~ok).sum())} illegal values; first at position {POSITIONS[r]} column {c}: got {got[r, c].item()!r}, "
                                 f"legal [{L.lo[r, c].item()!r}, {L.hi[r, c].item()!r}]")
        print(f"rope_table {name} half {half}: ambiguous share {L.share():.4f}")
        assert L.share() <= MAX_SHARE
    # equal positions give equal rows; position 0 is cos 1, sin 0
    assert torch.equal(cos[12], cos[13]) and torch.equal(sin[16], sin[17]) and torch.equal(cos[0], cos[-1])
    assert bool((cos[0] == 1).all()) and bool((sin[0] == 0).all())
    # the into form writes the same bits into caller-owned buffers
    c2, s2 = torch.empty_like(cos, device=DEV), torch.empty_like(sin, device=DEV)
    ops().rope_table_into(pos.to(DEV), inv.to(DEV), c2, s2)
    assert torch.equal(R.bits(c2.cpu()), R.bits(cos)) and torch.equal(R.bits(s2.cpu()), R.bits(sin))


# ------------------------------------------------------------------------------------------------------------
# qknorm_rope
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", [0, 1])
@pytest.mark.parametrize("nq,nkv", [(28, 4), (4, 1), (3, 3), (5, 2)])          # nq + nkv = 0, 1, 2, 3 mod 4 (four heads per step)
@pytest.mark.parametrize("hd,dp", [(128, 128), (64, 64), (32, 64)])
def test_qknorm_rope(hd, dp, nq, nkv, gen):
    """ld wider than the heads; V heads, pad lanes, trailing columns and the row past the last must keep their bits."""
    rows = 5 + (nq + nkv) % 3
    for family in ("exact", "tables", "castpoint", "tiny"):
        for use_norm in (0, 1):
            if family == "exact" and not use_norm:
                continue
            routes = (None, "mixed", "zeros", "ones") if family == "exact" else (("mixed",) if gen and use_norm else (None,))
            for routed in routes:
                case = R.qk_case(family, rows, nq, nkv, hd, dp, gen, use_norm, routed=routed)
                got = R.run_qknorm(ops(), case)
                _report(case, R.check(case.name, got, case.qkv0, case.region, R.qk_legal(case)))


def test_qknorm_rope_no_rows():
    case = R.qk_case("tables", 0, 4, 1, 64, 64, 0, 0)
    assert torch.equal(R.bits(R.run_qknorm(ops(), case)), R.bits(case.qkv0))


@pytest.mark.parametrize("use_norm", [0, 1])
def test_qknorm_rope_modes_are_distinguished(use_norm):
    """The und result must fail the gen check and the gen result the und check (castpoint family)."""
    got = {}
    for gen in (0, 1):
        case = R.qk_case("castpoint", 9, 5, 2, 128, 128, gen, use_norm)
        got[gen] = (case, R.run_qknorm(ops(), case))
        R.check(case.name, got[gen][1], case.qkv0, case.region, R.qk_legal(case))
    for gen in (0, 1):
        case = got[gen][0]
        assert not R.passes(case.name, got[1 - gen][1], case.qkv0, case.region, R.qk_legal(case)), f"gen_mode = {1 - gen} output passes the gen_mode = {gen} check"


# ------------------------------------------------------------------------------------------------------------
# decode_qkv_post
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nkv", [(28, 4), (3, 1), (12, 2)])                  # nq + 2 nkv = 36, 5, 16: 16 heads per block
@pytest.mark.parametrize("hd,dp", [(128, 128), (64, 64), (32, 64)])
def test_decode_qkv_post(hd, dp, nq, nkv):
    """kv_len 0, 63, 64, 127 in one batch on scattered pages, pools pre-filled with a sentinel: q in place, the K and V rows at their physical row with
    zero pad lanes, every other pool row untouched."""
    for family in ("exact", "tables", "castpoint", "tiny"):
        for use_norm in (0, 1):
            if family == "exact" and not use_norm:
                continue
            dc = R.DecodeCase(family, nq, nkv, hd, dp, use_norm)
            share = R.check_decode(dc, R.run_decode(ops(), dc))
            print(f"{dc.name}: ambiguous share {share:.4f}")
            assert share <= MAX_SHARE and (share == 0.0 or (use_norm and family != "exact"))


# ------------------------------------------------------------------------------------------------------------
# rope2d
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tables", "oracle"])
@pytest.mark.parametrize("hd,pad", [(72, 0), (72, 8), (64, 0), (64, 64), (16, 0), (16, 16)])
def test_rope2d(hd, pad, kind):
    """nheads counts the q and k heads; the V heads, pad lanes, trailing columns and the row past the last hold sentinels.  Bit-exact."""
    for rows in (9, 1):
        case = R.Rope2dCase(kind, rows, 6, hd, hd + pad)
        want, _ = R.emu_rope2d(case)
        got = R.run_rope2d(ops(), case)
        bad = R.bits(got) != R.bits(want)
        if bool(bad.any()):
            r, c = bad.nonzero()[0].tolist()
            raise AssertionError(f"{case.name}: {int(bad.sum())} elements differ; first at row {r} column {c} (head {c // case.dp}, lane {c % case.dp}): "
                                 f"got {got[r, c].item()!r} expected {want[r, c].item()!r}")
        print(f"{case.name}: bit-equal")
