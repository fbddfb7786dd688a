"""The designed GEMM inputs of tests/util_gemm_ref.py on the ping-pong kernel (variant 3), the persistent kernel (4) and its SGPR-base
form (5) under the grid this PROCESS was started with (BAGEL_GEMM_PERSIST_WGS / BAGEL_GEMM_SPLITK are read once per process):
exact families bit for bit, real-valued ones inside the per-element bound, four repeats of every persistent launch bit-identical, and
the number of K parts every persistent launch wrote into the K-split workspace (0: it ran unsplit) reported beside it.  One JSON line per case, then
ALL DESIGNED OK.   python tools/gemm_designed_check.py FAMILY[,FAMILY..]   (run by tests/test_gemm_designed_gpu.py)"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bagel_amd import ops  # noqa: E402
from tests import util_gemm_ref as R  # noqa: E402

DEV = "cuda"
SHAPES = [(1100, 264, 704), (1100, 264, 1152), (1100, 520, 1152), (257, 264, 1024)]
EPIS = ("plain", "bias", "res", "bias_res", "bias_gelu", "swiglu", "groups", "gather")
REPEATS = 4


def parts_written(ws):
    """K parts the launch just made left in the (NaN-filled) workspace: a split launch writes one 256 x 256 fp32 partial tile per leftover tile
    and K part (gemm.hip `(f32x4_t*)p.part + (long)w * (32 * 512)`), an unsplit one never touches it.  -> (parts, they fill the first slots)."""
    used = (~torch.isnan(ws)).view(-1, 256 * 256).any(1)
    n = int(used.sum())
    return n, bool(used[:n].all())


def main():
    families = sys.argv[1].split(",")
    good = True
    ws = ops._gemm_workspace(torch.zeros(1, device=DEV).device)                      # the one ops.gemm passes for this device and stream (unused with BAGEL_GEMM_SPLITK=0)
    for family in families:
        for M, N, K in SHAPES:
            for epi in EPIS:
                Nn = (N + 31) // 32 * 32 if epi == "swiglu" else N
                case = R.build(family, M, Nn, K, epi)
                ref = R.reference(case)
                args = R.gemm_args(case, DEV)
                rec = dict(family=family, epi=epi, shape=[M, Nn, K], worst=0.0, parts={})
                try:
                    first = R.run_gemm(ops, case, args, 3)
                    rec["worst"] = R.assert_case(case, first, ref, what="variant 3")
                    for variant in (4, 5):
                        # what the launcher did, observed: the workspace ops.gemm hands it is filled with NaN before the first repeat
                        ws.fill_(float("nan"))
                        outs = [R.run_gemm(ops, case, args, variant)]
                        n, packed = parts_written(ws)
                        assert packed, f"variant {variant}: the K parts are not in the first {n} workspace slots"
                        rec["parts"][str(variant)] = n
                        outs += [R.run_gemm(ops, case, args, variant) for _ in range(REPEATS - 1)]
                        assert all(torch.equal(R.bits(outs[0]), R.bits(o)) for o in outs[1:]), f"variant {variant}: repeats differ"
                        q = R.assert_case(case, outs[0], ref, what=f"variant {variant}")
                        rec["worst"] = max(rec["worst"], q)
                        if case.exact:
                            assert torch.equal(R.bits(outs[0]), R.bits(first)), f"variant {variant} differs from variant 3 on exact inputs"
                    rec["sha"] = hashlib.sha1(R.bits(outs[0]).numpy().tobytes()).hexdigest()      # of variant 5
                    rec["ok"] = True
                except AssertionError as e:
                    rec["ok"], rec["error"] = False, str(e)[:600]
                    good = False
                print(json.dumps(rec), flush=True)
    torch.cuda.synchronize()
    print("ALL DESIGNED OK" if good else "DESIGNED MISMATCH", flush=True)
    sys.exit(0 if good else 1)


if __name__ == "__main__":
    main()
