"""CPU restatement of the FP8 (OCP e4m3) option of the gen-expert GEMMs -- TEST INFRASTRUCTURE ONLY.

There is no reference implementation to pin against: the reference's quantised modes (app.py:114-131) are bitsandbytes NF4 / LLM.int8 on
CUDA, un-vendored; what the row in SURVEY.md 8f.4 asks for on MI355X is the chip's own low-precision MFMA path.  This file states the
scheme the kernels implement so the tests can check them bit for bit (quantiser) and to fp32-accumulation accuracy (GEMM):

    scale[r]  = max_k |x[r, k]| / 448                    (448 = largest finite e4m3fn value)
    q[r, k]   = e4m3fn(round-to-nearest-even(x[r, k] * (1 / scale[r])))
    C[m, n]   = epilogue( (sa[m] * sw[n]) * sum_k q_a[m, k] * q_w[n, k] )        fp32 accumulation, epilogues of the bf16 GEMM

DELAYED scaling of the SwiGLU output (round 6; the down projection's input inside a denoise loop -- ``DelayedScales`` below): the gate/up GEMM's epilogue writes the
e4m3 bytes itself, so a row's scale has to exist before its values do:

    scale_t[r] = margin * amax_{t-1}[r] / 448     (margin = 2; 1.0 where amax_{t-1}[r] = 0; NaN where it is NaN or Inf),    amax_t[r] = max_k |x_t[r, k]|
    q_t[r, k]  = e4m3fn(rne(clamp(x_t[r, k] * (1 / scale_t[r]), -448, 448)))      (only finite values are clamped: NaN / Inf stay NaN codes)

with amax_{t-1} the row maxima the SAME rows left in the forward of the IMMEDIATELY PRECEDING Euler step, quantised with the same state.  Without such a
history (the first step, the first full step after TaylorSeer steps, a step where cfg_interval switches between the stream-batched state and the per-stream
ones) the forward uses the exact row-wise scale above and leaves amax = (max|row| / 448) * 448 (what the product reconstructs from the exact scale).
The exact quantiser's row maximum ignores NaN (fmaxf), so a NaN value gives a NaN code under a finite scale; an Inf makes the scale Inf and the codes NaN / 0.
"""
import torch


def quantize_rows_fp8(x):
    """bf16 / fp32 [rows, K] -> (uint8 view of float8_e4m3fn [rows, K], fp32 scale [rows]) exactly as bagel_quantize_rows_fp8:
    fp32 reciprocal, fp32 product, round-to-nearest-even conversion."""
    xf = x.float()
    a = xf.abs()
    amax = torch.where(torch.isnan(a), torch.zeros_like(a), a).amax(dim=1)          # fmaxf: a NaN does not become the row maximum
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    inv = 1.0 / scale
    q = (xf * inv[:, None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale


def dequant(q_u8, scale):
    return q_u8.view(torch.float8_e4m3fn).float() * scale[:, None]


def gemm_fp8(qa, sa, qw, sw, bias=None, residual=None, swiglu=False):
    """fp32 product of the de-quantised operands with the epilogue roundings of the bf16 GEMM (tests/test_ops_gpu.py::ref_gemm)."""
    acc = (qa.view(torch.float8_e4m3fn).float() @ qw.view(torch.float8_e4m3fn).float().t()) * (sa[:, None] * sw[None, :])
    if swiglu:
        N = qw.shape[0]
        a = acc.view(acc.shape[0], N // 32, 2, 16)
        g = a[:, :, 0].reshape(acc.shape[0], -1).to(torch.bfloat16)
        u = a[:, :, 1].reshape(acc.shape[0], -1).to(torch.bfloat16)
        return torch.nn.functional.silu(g) * u
    if bias is not None:
        acc = acc + bias.float()
    c = acc.to(torch.bfloat16)
    if residual is not None:
        c = residual + c
    return c


def delayed_scales(prev, margin=2.0):
    """bagel_fp8_delayed_scales: the scale the row maxima of the previous step give (1.0 for 0, NaN for NaN / Inf)."""
    k = torch.tensor(margin, dtype=torch.float32) / torch.tensor(448.0, dtype=torch.float32)
    return torch.where(torch.isfinite(prev), torch.where(prev > 0, prev * k, torch.ones_like(prev)), torch.full_like(prev, float("nan")))


def quantize_rows_delayed(x, scale):
    """The fp8-output epilogue of bagel_gemm_fp8_swiglu_q8: (uint8 codes, fp32 row maxima (NaN-propagating)) of x under the caller's row scales."""
    xf = x.float()
    y = xf * (1.0 / scale)[:, None]
    ok = torch.isfinite(xf) & ~torch.isnan(y)
    q = torch.where(ok, y.clamp(-448.0, 448.0), torch.full_like(y, float("nan"))).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), xf.abs().amax(dim=1)


class DelayedScales:
    """Restates bagel_amd.modeling.bagel.qwen2_navit.Fp8DelayedScales (its rule included) + the fp8-output epilogue of bagel_gemm_fp8_swiglu_q8 +
    bagel_fp8_delayed_scales for the oracle's sequential forwards.  The history of a (weight, state, stream) triple is the history of one forward stream's
    rows at one layer in one of the product's states: state 3 is the stream-batched forward, 0 / 1 / 2 the per-stream ones (cond / cfg-text / cfg-img).
    ``ptrs``: data_ptr()s of the weights whose INPUT is quantised this way (the gen expert's down projections), in layer order.  ``begin_step(i, batched)``
    once per Euler step (``batched``: the product runs this step's streams as ONE forward -- model.cfg_batched with CFG on); ``select(stream)`` in front of
    each stream's forward.  ``trace``: one (step, stream, layer, "exact" | "delayed", age) per quantisation, age = steps since these rows were last quantised
    (None: never)."""

    def __init__(self, ptrs, margin=2.0):
        self.layer = {p: li for li, p in enumerate(ptrs)}
        self.ptrs, self.margin = set(self.layer), float(margin)
        self.hist, self.last, self.trace = {}, {}, []
        self.step, self.batched, self.stream = -1, False, 0

    def begin_step(self, step=None, batched=False):
        self.step = self.step + 1 if step is None else int(step)
        self.batched, self.stream = bool(batched), 0

    def select(self, stream):
        self.stream = int(stream)

    def quantize(self, key, x):
        s = self.stream
        hk = (key, 3 if self.batched else s, s)
        prev = self.hist.get(hk)
        last = self.last.get((key, s))
        self.last[(key, s)] = self.step
        age = None if last is None else self.step - last
        if prev is None or prev[0] != self.step - 1:       # no history from the previous step: the exact scheme; the product keeps scale * 448 as the maxima
            q, scale = quantize_rows_fp8(x)
            self.hist[hk] = (self.step, scale * torch.tensor(448.0))
            self.trace.append((self.step, s, self.layer[key], "exact", age))
            return q, scale
        scale = delayed_scales(prev[1], self.margin)
        q, amax = quantize_rows_delayed(x, scale)
        self.hist[hk] = (self.step, amax)
        self.trace.append((self.step, s, self.layer[key], "delayed", age))
        return q, scale


def down_proj_gen_ptrs(W):
    """The weights whose input the product quantises with DELAYED scales: the gen expert's down projections, in layer order."""
    sel = [(int(k.split("language_model.model.layers.")[1].split(".")[0]), v.data_ptr()) for k, v in W.items()
           if "language_model.model.layers." in k and k.endswith("mlp_moe_gen.down_proj.weight")]
    return [p for _, p in sorted(sel)]
