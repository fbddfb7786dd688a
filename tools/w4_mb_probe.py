"""Same-box, same-process measurement of batched decode on MXFP4 weights (csrc/gemv_mb_w4.hip) beside what the project already has.  Needs a GPU.

    python tools/w4_mb_probe.py [--batches 8,16,32] [--ctx 4936] [--layers 28] [--iters 24] [--legs step,proj] [--out profiles/w4_mb_probe.json]

Step leg: BAGEL-7B-MoT geometry, random weights, B requests on ctx-key contexts (random K/V rows: a decode step's cost does not depend on their values).  Three
DecodeSessions over the same context -- bf16 weights on gemv_mb, MXFP4 weights on the new stream, MXFP4 weights on the gemm_w4 fallback (BAGEL_GEMV_MB_W4=0
while that session captures) -- each captured into its hipGraph; after warm-up the three are replayed ALTERNATELY, one step each per round, and the median /
min / max ms per replayed step over >= 20 rounds is reported.
Projection leg: the four projections of a layer at M = B, median us of >= 20 launches each (device events) of: the bf16 route of the session (gemv_mb, with the
RMSNorm fused or in front as decode.py routes it), the activation quantiser, gemv_mb_w4 alone, gemm_w4 alone; achieved TB/s of the stream over its algorithmic
bytes (codes + scale bytes + e4m3 activations + bf16 output).
Prints ONE JSON line.  MXFP4 weights change results: every figure here is reported beside, never as, the bf16 headline of bench.py."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROJ = [("qkv", 4608, 3584, "norm_bias"), ("o", 3584, 3584, "residual"), ("gate_up", 37888, 3584, "norm_swiglu"), ("down", 3584, 18944, "residual")]


def spread(ts):
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def timed_us(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return spread(ts)


def proj_leg(B, iters):
    from bagel_amd import ops
    dev = torch.device("cuda")
    rows = []
    for name, N, K, kind in PROJ:
        g = torch.Generator(device=dev).manual_seed(N + K + B)
        x = (torch.randn(B, K, device=dev, generator=g) * 1.5).to(torch.bfloat16)
        W = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
        nw = torch.ones(K, dtype=torch.bfloat16, device=dev)
        swiglu, norm = kind.endswith("swiglu"), kind.startswith("norm")
        Nout = N // 2 if swiglu else N
        epi = ops.EPI_SWIGLU16 if swiglu else ops.EPI_NONE
        C = torch.zeros((B, Nout), dtype=torch.bfloat16, device=dev)
        R = torch.zeros((B, Nout), dtype=torch.bfloat16, device=dev) if kind == "residual" else None
        bias = torch.zeros(N, dtype=torch.bfloat16, device=dev) if kind == "norm_bias" else None
        h = torch.empty_like(x)
        aq, sa = torch.empty((B, K), dtype=torch.uint8, device=dev), torch.empty((B,), dtype=torch.float32, device=dev)
        w4, s4 = ops.quantize_rows_mxfp4(W)
        ws = torch.empty(max(ops.mb_workspace_floats(N, K), ops.mb_w4_workspace_floats(N, K), 4), dtype=torch.float32, device=dev)

        def bf16_route():
            if norm and B > 16:
                ops.rmsnorm(x, nw, h, 1e-6)
                return ops.gemv_mb(h, W, C, bias=bias, epilogue=epi, M=B, workspace=ws)
            return ops.gemv_mb(x, W, C, bias=bias, residual=R, epilogue=epi, M=B, norm_w=nw if norm else None, eps=1e-6, workspace=ws)

        def quantiser():
            return ops.rmsnorm_fp8(x, nw, aq, sa, 1e-6) if norm else ops.quantize_rows_fp8(x, aq, sa)
        quantiser()
        row = dict(proj=name, N=N, K=K, M=B)
        row["bf16_gemv_mb_us"] = timed_us(bf16_route, iters)
        row["quantiser_us"] = timed_us(quantiser, iters)
        row["gemv_mb_w4_us"] = timed_us(lambda: ops.gemv_mb_w4(aq, sa, w4, s4, C, bias=bias, residual=R, epilogue=epi, M=B, workspace=ws), iters)
        row["gemm_w4_us"] = timed_us(lambda: ops.gemm_w4(aq, sa, w4, s4, C, bias=bias, residual=R, epilogue=epi, M=B), iters)
        nbytes = N * K // 2 + N * K // 32 + B * K + B * Nout * 2
        row["stream_bytes"] = nbytes
        row["stream_tb_s"] = nbytes / (row["gemv_mb_w4_us"]["median"] * 1e-6) / 1e12
        row["bf16_bytes"] = N * K * 2 + B * K * 2 + B * Nout * 2
        rows.append(row)
        sys.stderr.write(json.dumps(row) + "\n")
        del x, W, w4, s4, C, ws
    tot = lambda k: sum(r[k]["median"] for r in rows)  # noqa: E731
    return dict(rows=rows, bf16_projections_us=tot("bf16_gemv_mb_us"), w4_stream_projections_us=tot("gemv_mb_w4_us") + tot("quantiser_us"),
                w4_fallback_projections_us=tot("gemm_w4_us") + tot("quantiser_us"))


def synthetic_context(model, B, ctx):
    """A NaiveCache holding B contexts of ctx random keys per layer, without the prefill that would write them (this reaches into the container's storage
    fields: the merged [ctx_0 | ctx_1 | ...] layout DecodeSession adopts)."""
    from bagel_amd.modeling.bagel.qwen2_navit import NaiveCache
    eng = model.language_model.engine(check=True)
    L = len(eng.layers)
    c = NaiveCache(L)
    g = torch.Generator(device=eng.device).manual_seed(4)
    for i in range(L):
        c._k[i] = (torch.randn(B * ctx, eng.nkv * eng.dp, device=eng.device, generator=g) * 0.5).to(torch.bfloat16)
        c._v[i] = (torch.randn(B * ctx, eng.nkv * eng.dp, device=eng.device, generator=g) * 0.5).to(torch.bfloat16)
        c._lens[i] = [ctx] * B
    c._total, c._nkv, c._hd, c._dp = B * ctx, eng.nkv, eng.hd, eng.dp
    return c


def step_leg(model, B, ctx, iters, warmup=4):
    from bagel_amd.modeling.bagel.decode import DecodeSession
    lm = model.language_model
    eng = lm.engine(check=True)
    cache = synthetic_context(model, B, ctx)
    start = torch.randint(0, 150000, (B,), generator=torch.Generator().manual_seed(5))
    pos = torch.full((B,), ctx, dtype=torch.long)
    sessions = {}
    for case, wq, knob in (("bf16_gemv_mb", None, None), ("mxfp4_stream", "mxfp4", None), ("mxfp4_gemm_w4_fallback", "mxfp4", "0")):
        if knob is not None:
            os.environ["BAGEL_GEMV_MB_W4"] = knob
        try:
            s = DecodeSession(eng, lm.model.embed_tokens.weight.data, lm.lm_head.weight.data, cache, [ctx] * B, start, pos, warmup + iters + 2, weight_quant=wq)
            s.step(None)                                       # eager: lazily enabled kernels, workspaces
            if not s.capture(include_advance=True):
                raise RuntimeError(f"{case}: hipGraph capture failed: {s.graph_error}")
        finally:
            os.environ.pop("BAGEL_GEMV_MB_W4", None)
        sessions[case] = s
    ts = {k: [] for k in sessions}
    for it in range(warmup + iters):
        for case, s in sessions.items():                       # alternated: one replayed step each per round
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s.step(None)
            e1.record()
            e1.synchronize()
            if it >= warmup:
                ts[case].append(e0.elapsed_time(e1))
    out = dict(B=B, ctx=ctx, layers=len(eng.layers), ms_per_step={k: spread(v) for k, v in ts.items()})
    out["tokens_per_s"] = {k: B / (v["median"] * 1e-3) for k, v in out["ms_per_step"].items()}
    sys.stderr.write(json.dumps(out) + "\n")
    del sessions, cache
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,16,32")
    ap.add_argument("--ctx", type=int, default=4936)
    ap.add_argument("--layers", type=int, default=None, help="decoder layers of the step leg (default: all 28)")
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--legs", default="step,proj")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("w4_mb_probe needs a GPU (bagel_amd has no CPU path)")
    iters = max(20, a.iters)
    batches = [int(x) for x in a.batches.split(",")]
    res = {"tool": "w4_mb_probe", "device": torch.cuda.get_device_name(0), "note": "MXFP4 weights change results: reported beside the bf16 headline, never as it"}
    with torch.no_grad():
        if "proj" in a.legs:
            res["projections"] = {str(B): proj_leg(B, iters) for B in batches}
        if "step" in a.legs:
            from bagel_amd.factory import BAGEL_7B_MOT, build_bagel, init_random_
            model, _ = build_bagel(BAGEL_7B_MOT, device=torch.device("cuda"), num_layers=a.layers, with_vae=False)
            init_random_(model, seed=0)
            res["steps"] = [step_leg(model, B, a.ctx, iters) for B in batches]
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
