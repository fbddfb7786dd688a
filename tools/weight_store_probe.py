"""Same-box, same-process measurement of the whole-model load mode weight_store = "mxfp4" beside the modes the project already has.

    python tools/weight_store_probe.py [--legs gemm,model] [--layers N] [--iters 20] [--m 32768,4098] [--out profiles/weight_store_probe.json]

GEMM leg: at the 7B shapes (K, N) = (3584, 4608), (3584, 3584), (3584, 37888 SwiGLU), (18944, 3584) and M = 32 768 / 4 098, median of >= 20 timed launches
(device events, after warm-up, fresh random operands per shape) of: ops.gemm (bf16), ops.dequantize_nf4 + ops.gemm (what the NF4 mode pays per layer and
projection), ops.gemm_fp8, ops.gemm_w4.
Model leg: 7B geometry, random weights, one 1024^2 text->image request at 4 images per batch for a few Euler steps (ms per step, peak bytes) in bf16, "nf4"
and "mxfp4"; batch-1 decode tok/s in "nf4", in "mxfp4" as a whole-model mode, and with weight_quant="mxfp4" on the bf16 engine (same kernels, same codes).
Prints ONE JSON line.  The quantised modes change results: every figure here is reported beside, never as, the bf16 headline of bench.py."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(3584, 4608, False), (3584, 3584, False), (3584, 37888, True), (18944, 3584, False)]


def timed(fn, iters, warmup=5):
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
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def gemm_leg(ms, iters):
    from bagel_amd import ops
    dev = torch.device("cuda")
    out = []
    for K, N, swiglu in SHAPES:
        for M in ms:
            g = torch.Generator(device=dev).manual_seed(K + N + M)
            A = (torch.randn(M, K, device=dev, generator=g) * 1.5).to(torch.bfloat16)
            W = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
            Nout = N // 2 if swiglu else N
            C = torch.empty((M, Nout), dtype=torch.bfloat16, device=dev)
            epi = ops.EPI_SWIGLU16 if swiglu else ops.EPI_NONE
            aq, sa = ops.quantize_rows_fp8(A)
            w8, s8 = ops.quantize_rows_fp8(W)
            w4, s4 = ops.quantize_rows_mxfp4(W)
            qn, an = ops.quantize_nf4(W)
            scratch = torch.empty_like(W)
            row = dict(K=K, N=N, M=M, swiglu=swiglu)
            row["bf16_ms"] = timed(lambda: ops.gemm(A, W, C, epilogue=epi), iters)
            row["nf4_dequant_ms"] = timed(lambda: ops.dequantize_nf4(qn, an, scratch), iters)
            row["nf4_path_ms"] = timed(lambda: (ops.dequantize_nf4(qn, an, scratch), ops.gemm(A, scratch, C, epilogue=epi)), iters)
            row["fp8_ms"] = timed(lambda: ops.gemm_fp8(aq, sa, w8, s8, C, epilogue=epi), iters)
            row["w4_ms"] = timed(lambda: ops.gemm_w4(aq, sa, w4, s4, C, epilogue=epi), iters)
            row["w4_tflops"] = 2.0 * M * N * K / row["w4_ms"] / 1e9
            row["w4_le_nf4_path"] = row["w4_ms"] <= row["nf4_path_ms"]
            out.append(row)
            sys.stderr.write(json.dumps(row) + "\n")
            del A, W, C, aq, sa, w8, s8, w4, s4, qn, an, scratch
    return out


class FixedTokenizer:
    def __init__(self, ids):
        self.ids = list(ids)

    def encode(self, text):
        return list(self.ids)


def model_leg(layers, steps, decode_tokens):
    from bagel_amd.factory import BAGEL_7B_MOT, NEW_TOKEN_IDS_QWEN25, build_bagel, init_random_
    from bagel_amd.modeling.bagel.qwen2_navit import NaiveCache
    cfg, ids = BAGEL_7B_MOT, NEW_TOKEN_IDS_QWEN25
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1)
    tok = FixedTokenizer(torch.randint(0, 151643, (32,), generator=g).tolist())
    B, sizes = 4, [(1024, 1024)] * 4
    out = {}
    for mode in ("bf16", "nf4", "mxfp4"):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        model, _ = build_bagel(cfg, device=dev, num_layers=layers, with_vae=False)
        init_random_(model, seed=0)
        model.llm2vae.weight.data.normal_(0, cfg["llm"]["hidden_size"] ** -0.5, generator=torch.Generator(device=dev).manual_seed(1))
        L = model.config.llm_config.num_hidden_layers
        row = {"layers": L}
        if mode != "bf16":
            row["resident_gb"] = model.quantize_language_model(mode) / 1e9
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()

        def denoise(T):
            gi, lens, ropes = model.prepare_prompts([0] * B, [0] * B, ["p"] * B, tok, ids)
            cache = model.forward_cache_update_text(NaiveCache(L), **gi)
            torch.manual_seed(3)
            li = model.prepare_vae_latent(lens, ropes, sizes, ids)
            ci = model.prepare_vae_latent_cfg([0] * B, [0] * B, sizes)
            kw = {f"cfg_text_{k[4:]}": v for k, v in ci.items()}
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            model.generate_image(past_key_values=cache, cfg_text_past_key_values=NaiveCache(L), num_timesteps=T, timestep_shift=3.0, cfg_text_scale=4.0,
                                 cfg_interval=[0.0, 1.0], cfg_renorm_min=0.0, cfg_renorm_type="global", **kw, **li)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / (T - 1)
        denoise(2)                                             # warm-up: workspaces, plans, lazily enabled kernels
        row["ms_per_step"] = denoise(steps + 1)
        row["peak_gb"] = torch.cuda.max_memory_allocated() / 1e9
        model.language_model.engine().release_workspaces()

        def decode(weight_quant=None):
            gi, lens, ropes = model.prepare_prompts([0], [0], ["p"], tok, ids)
            cache = model.forward_cache_update_text(NaiveCache(L), **gi)
            st = model.prepare_start_tokens(lens, ropes, ids)
            best = 0.0
            for _ in range(2):                                 # first call captures the graph
                import copy
                c = copy.deepcopy(cache)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                model.generate_text(past_key_values=c, max_length=decode_tokens, do_sample=False, end_token_id=None, weight_quant=weight_quant, **st)
                e1.record()
                e1.synchronize()
                best = max(best, decode_tokens / (e0.elapsed_time(e1) / 1e3))
            return best
        if mode == "bf16":
            row["decode_tok_s_weight_quant_mxfp4"] = decode("mxfp4")
        else:
            row["decode_tok_s"] = decode()
        out[mode] = row
        sys.stderr.write(json.dumps({mode: row}) + "\n")
        del model
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="gemm,model")
    ap.add_argument("--layers", type=int, default=None, help="decoder layers of the model leg (default: all 28)")
    ap.add_argument("--steps", type=int, default=3, help="timed Euler steps of the model leg")
    ap.add_argument("--decode-tokens", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--m", default="32768,4098")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"tool": "weight_store_probe", "device": torch.cuda.get_device_name(0),
           "note": "weight_store options change results: reported beside the bf16 headline, never as it"}
    with torch.no_grad():
        if "gemm" in a.legs:
            res["gemm"] = gemm_leg([int(x) for x in a.m.split(",")], max(20, a.iters))
        if "model" in a.legs:
            res["model"] = model_leg(a.layers, a.steps, a.decode_tokens)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
