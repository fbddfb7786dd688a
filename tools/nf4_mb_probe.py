"""Same-box, same-process measurement of batched decode on NF4 weights (csrc/gemv_mb_nf4.hip) beside what the project already has.  Needs a GPU.

    python tools/nf4_mb_probe.py [--batches 16,32] [--proj-batches 5,8,16,32] [--ctx 4936] [--layers 28] [--iters 24] [--legs step,proj] [--out profiles/nf4_mb_probe.json]

Step leg: BAGEL-7B-MoT geometry, random weights, B requests on ctx-key contexts (random K/V rows: a decode step's cost does not depend on their values).  Three
DecodeSessions over the same context -- bf16 weights on gemv_mb (context), NF4 weights on the new stream, NF4 weights on the parent route (gemv_nf4 in passes of
four rows: BAGEL_GEMV_MB_NF4=0 while that session captures) -- each captured into its hipGraph; after warm-up the three are replayed ALTERNATELY, one step each per
round, and the median / min / max ms per replayed step over >= 20 rounds is reported.
Projection leg: the four projections of a layer at M = B, median us of >= 20 launches each (device events) of: the bf16 route of the session (gemv_mb, with the
RMSNorm fused or in front as decode.py routes it), the RMSNorm launch the stream needs, gemv_mb_nf4 alone, the parent route gemv_nf4 (RMSNorm fused); achieved
bytes/s of the stream over the code + absmax bytes and its share of the 8 TB/s HBM specification.
Prints ONE JSON line on stdout and the log lines of profiles/nf4_mb_probe.log on stderr.  NF4 weights change results: every figure here is reported beside,
never as, the bf16 headline of bench.py."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROJ = [("qkv", 4608, 3584, "norm_bias"), ("o", 3584, 3584, "residual"), ("gate_up", 37888, 3584, "norm_swiglu"), ("down", 3584, 18944, "residual")]
HBM_SPEC = 8.0e12


def spread(ts):
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def fmt(s, digits=1):
    return f"{s['median']:.{digits}f} ({s['min']:.{digits}f}-{s['max']:.{digits}f})"


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
        q4, am = ops.quantize_nf4(W)
        ws = torch.empty(max(ops.mb_workspace_floats(N, K), ops.mb_nf4_workspace_floats(N, K), 4), dtype=torch.float32, device=dev)

        def bf16_route():
            if norm and B > 16:
                ops.rmsnorm(x, nw, h, 1e-6)
                return ops.gemv_mb(h, W, C, bias=bias, epilogue=epi, M=B, workspace=ws)
            return ops.gemv_mb(x, W, C, bias=bias, residual=R, epilogue=epi, M=B, norm_w=nw if norm else None, eps=1e-6, workspace=ws)
        ops.rmsnorm(x, nw, h, 1e-6)
        row = dict(proj=name, N=N, K=K, M=B)
        row["bf16_gemv_mb_us"] = timed_us(bf16_route, iters)
        row["rmsnorm_us"] = timed_us(lambda: ops.rmsnorm(x, nw, h, 1e-6), iters) if norm else None
        row["gemv_mb_nf4_us"] = timed_us(lambda: ops.gemv_mb_nf4(h if norm else x, q4, am, C, bias=bias, residual=R, epilogue=epi, M=B, workspace=ws), iters)
        row["gemv_nf4_parent_us"] = timed_us(lambda: ops.gemv_nf4(x, q4, am, C, bias=bias, residual=R, epilogue=epi, M=B, norm_w=nw if norm else None, eps=1e-6), iters)
        nbytes = N * K // 2 + N * (K // 64) * 4
        row["code_absmax_bytes"] = nbytes
        row["stream_bytes_per_s"] = nbytes / (row["gemv_mb_nf4_us"]["median"] * 1e-6)
        row["share_of_hbm_spec"] = row["stream_bytes_per_s"] / HBM_SPEC
        rows.append(row)
        sys.stderr.write(f"B={B:2d} {name:8s} N={N:5d} K={K:5d}  bf16 gemv_mb {fmt(row['bf16_gemv_mb_us'])}  rmsnorm {fmt(row['rmsnorm_us']) if norm else '-'}  "
                         f"gemv_mb_nf4 {fmt(row['gemv_mb_nf4_us'])}  parent gemv_nf4 {fmt(row['gemv_nf4_parent_us'])}  stream {row['stream_bytes_per_s'] / 1e12:.2f} TB/s "
                         f"over {nbytes / 1e6:.1f} MB of codes + absmax = {100 * row['share_of_hbm_spec']:.1f} % of the 8 TB/s HBM spec\n")
        del x, W, q4, am, C, ws
    tot = lambda k: sum(r[k]["median"] for r in rows if r[k] is not None)  # noqa: E731
    out = dict(rows=rows, bf16_projections_us=tot("bf16_gemv_mb_us"), nf4_stream_projections_us=tot("gemv_mb_nf4_us") + tot("rmsnorm_us"),
               nf4_parent_projections_us=tot("gemv_nf4_parent_us"))
    sys.stderr.write(f"B={B:2d} four projections: bf16 {out['bf16_projections_us']:.1f}  rmsnorm + stream {out['nf4_stream_projections_us']:.1f}  "
                     f"parent gemv_nf4 {out['nf4_parent_projections_us']:.1f}\n")
    return out


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
    for case, wq, knob in (("bf16_gemv_mb", None, None), ("nf4_stream", "nf4", None), ("nf4_parent_gemv_nf4", "nf4", "0")):
        if knob is not None:
            os.environ["BAGEL_GEMV_MB_NF4"] = knob
        try:
            s = DecodeSession(eng, lm.model.embed_tokens.weight.data, lm.lm_head.weight.data, cache, [ctx] * B, start, pos, warmup + iters + 2, weight_quant=wq)
            s.step(None)                                       # eager: lazily enabled kernels, workspaces
            if not s.capture(include_advance=True):
                raise RuntimeError(f"{case}: hipGraph capture failed: {s.graph_error}")
        finally:
            os.environ.pop("BAGEL_GEMV_MB_NF4", None)
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
    m = out["ms_per_step"]
    sys.stderr.write(f"B={B:2d}  " + "  ".join(f"{k} {fmt(v, 3)}" for k, v in m.items()) + "  tok/s " + " / ".join(f"{v:.0f}" for v in out["tokens_per_s"].values()) + "\n")
    del sessions, cache
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,32")
    ap.add_argument("--proj-batches", default="5,8,16,32")
    ap.add_argument("--ctx", type=int, default=4936)
    ap.add_argument("--layers", type=int, default=None, help="decoder layers of the step leg (default: all 28)")
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--legs", default="step,proj")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nf4_mb_probe needs a GPU (bagel_amd has no CPU path)")
    iters = max(20, a.iters)
    res = {"tool": "nf4_mb_probe", "device": torch.cuda.get_device_name(0), "note": "NF4 weights change results: reported beside the bf16 headline, never as it"}
    with torch.no_grad():
        if "proj" in a.legs:
            res["projections"] = {str(B): proj_leg(B, iters) for B in (int(x) for x in a.proj_batches.split(","))}
        if "step" in a.legs:
            from bagel_amd.factory import BAGEL_7B_MOT, build_bagel, init_random_
            model, _ = build_bagel(BAGEL_7B_MOT, device=torch.device("cuda"), num_layers=a.layers, with_vae=False)
            init_random_(model, seed=0)
            res["steps"] = [step_leg(model, B, a.ctx, iters) for B in (int(x) for x in a.batches.split(","))]
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
