"""CPU: the host logic of the whole-model load mode ``quantize_language_model("mxfp4")`` on the torch stand-ins of tests/mock_ops.py -- which weights are
stored as codes (all fourteen projections of every decoder layer, both experts), what is quantised where (norm output, attention output, SwiGLU output: e4m3
rows with exact scales), which expert serves which rows, and that the decode adopts the stored codes -- against the ORACLE with the MXFP4 scheme switched
into exactly those linears on every path (``O.MXFP4_WEIGHT_PTRS``; oracle/mxfp4.py states the product).  Both sides run the same torch arithmetic on one
host, so the bounds are the ones tests/test_host_logic_cpu.py::test_text_to_image_host_path_matches_reference uses for the same quantities."""
import pytest
import torch

from oracle import bagel_oracle as O
from oracle import mxfp4 as MX
from oracle.configs import TINY, TINY_D128, NEW_TOKEN_IDS_TINY, StubTokenizer
from tests import mock_ops
from tests.test_host_logic_cpu import _tokens_match, cfg_kwargs, cpu_model, new_cache, rel
from tests.util_models import oracle_weights

PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def natural_scales(Ws, K):
    """Device order of the scale bytes (oracle/mxfp4.py::permute_scales) -> natural [N, K/32], as tests/mock_ops.py::gemv_w4 undoes it."""
    N, ng = Ws.shape
    nk = K // 128
    return Ws.view(N, ng // 16, 4, 4).permute(0, 1, 3, 2).reshape(N, -1, 4)[:, :nk].reshape(N, nk * 4)


def gemm_w4(Aq, sa, Wq, Ws, C, *, bias=None, rows=None, M=None, residual=None, epilogue=0):
    """CPU stand-in of ops.gemm_w4: oracle/mxfp4.py::gemv_w4's product on ALREADY quantised rows, plus the row list and the residual."""
    if M is None:
        M = rows.numel() if rows is not None else Aq.shape[0]
    r = torch.arange(M) if rows is None else rows[:M].long()
    W = MX.dequant_mxfp4(Wq, natural_scales(Ws, Wq.shape[1] * 2))
    acc = (Aq[r].view(torch.float8_e4m3fn).float() @ W.t()) * sa[r][:, None]
    if epilogue == 3:
        a = acc.view(M, Wq.shape[0] // 32, 2, 16)
        g, u = a[:, :, 0].reshape(M, -1).to(torch.bfloat16), a[:, :, 1].reshape(M, -1).to(torch.bfloat16)
        y = torch.nn.functional.silu(g) * u
    else:
        if bias is not None:
            acc = acc + bias.float()
        y = acc.to(torch.bfloat16)
        if residual is not None:
            y = residual[r, :y.shape[1]] + y
    C[r, :y.shape[1]] = y
    return C


def install(monkeypatch):
    from bagel_amd import ops
    mock_ops.install(monkeypatch)
    monkeypatch.setattr(ops, "gemm_w4", gemm_w4, raising=False)


def all_projection_ptrs(W):
    """The fourteen projection weights of every decoder layer: both experts (``O.mxfp4_decode_weight_ptrs`` names the und expert only)."""
    out = set()
    for k, v in W.items():
        if "language_model.model.layers." in k and k.endswith(".weight") and any(f".{n}." in k or f".{n}_moe_gen." in k for n in PROJ):
            out.add(v.data_ptr())
    return out


def test_stand_in_is_the_restatement():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(9, 256, generator=g).to(torch.bfloat16)
    w = (torch.randn(64, 256, generator=g) * 0.1).to(torch.bfloat16)
    q, s = mock_ops.quantize_rows_mxfp4(w)
    aq, sa = mock_ops.quantize_rows_fp8(x)
    for swiglu in (False, True):
        C = torch.zeros(9, 32 if swiglu else 64, dtype=torch.bfloat16)
        gemm_w4(aq, sa, q, s, C, epilogue=3 if swiglu else 0)
        assert torch.equal(C, MX.gemv_w4(x, *MX.quantize_mxfp4(w), swiglu=swiglu))


def test_mxfp4_load_mode_matches_the_oracle_on_every_path(golden, monkeypatch):
    install(monkeypatch)
    monkeypatch.setenv("BAGEL_DECODE_GRAPH", "0")
    cfg = TINY_D128
    g = golden("tiny_d128_t2i")
    L = cfg["llm"]["num_hidden_layers"]
    tok = StubTokenizer(cfg["llm"]["vocab_size"])
    W, _ = oracle_weights(cfg)
    model = cpu_model(cfg)
    full = sum(p.numel() * 2 for n, p in model.language_model.model.layers.named_parameters() if "proj" in n and n.endswith("weight"))
    resident = model.quantize_language_model("mxfp4", release_bf16=True)
    assert model.language_model.engine().weight_store == "mxfp4"
    assert resident < 0.28 * full, (resident, full)                 # 4 bits + one byte per 32 weights = 0.266
    assert all(p.numel() == 0 for n, p in model.language_model.model.layers.named_parameters() if "proj" in n and n.endswith("weight"))
    P0 = model.language_model.engine().layers[0]
    assert all(isinstance(e, tuple) and e[0].dtype == torch.uint8 for name in ("wqkv", "wo", "wgu", "wd") for e in getattr(P0, name)), \
        "the forward is handed codes, never a materialised matrix"

    gi, newlens, newrope = model.prepare_prompts([0, 0], [0, 0], g["prompts"], tok, NEW_TOKEN_IDS_TINY)
    cache = model.forward_cache_update_text(new_cache(cfg), **gi)
    prefill = [(cache.key_cache[i].clone(), cache.value_cache[i].clone()) for i in range(L)]
    lat = model.generate_image(past_key_values=cache, **cfg_kwargs("cfg_text", new_cache(cfg), g["cfg_inputs"]), **g["gen_kwargs"], **g["latent_inputs"])
    st = model.prepare_start_tokens(newlens, newrope, NEW_TOKEN_IDS_TINY)
    n = 5
    toks = model.generate_text(past_key_values=cache, max_length=n, do_sample=False, end_token_id=None, **st)
    assert model._last_decode_session.weight_quant == "mxfp4"      # the decode streamed the stored codes

    # the oracle caches quantised weights by (data_ptr, version): entries of weight tensors an earlier test has since freed must not be found again
    O.linear.__dict__.pop("_mx", None)
    O.MXFP4_WEIGHT_PTRS = all_projection_ptrs(W)
    try:
        assert len(O.MXFP4_WEIGHT_PTRS) == 14 * L
        oc = O.forward_cache_update_text(W, cfg, O.OracleCache(L), **gi)
        ci = g["cfg_inputs"]
        cfgd = dict(cache=O.OracleCache(L), position_ids=ci["cfg_packed_position_ids"], query_indexes=ci["cfg_packed_query_indexes"],
                    key_values_lens=ci["cfg_key_values_lens"], key_value_indexes=ci["cfg_packed_key_value_indexes"])
        olat = O.generate_image(W, cfg, g["latent_inputs"], oc, cfg_text=cfgd, **g["gen_kwargs"])
        okv = [(oc.key_cache[i].clone(), oc.value_cache[i].clone()) for i in range(L)]
        otoks, ologits = O.generate_text(W, cfg, oc, st["packed_key_value_indexes"], st["key_values_lens"], st["packed_start_tokens"],
                                         st["packed_query_position_ids"], n, return_logits=True)
    finally:
        O.MXFP4_WEIGHT_PTRS = set()
        O.linear.__dict__.pop("_mx", None)
    for i in range(L):
        ek, ev = rel(prefill[i][0], okv[i][0]), rel(prefill[i][1], okv[i][1])
        print(f"layer {i}: K {ek:.3g} V {ev:.3g}")
        assert ek < 1e-2 and ev < 1e-2, f"prefill K/V layer {i}: {ek:.3g} {ev:.3g}"
    # the scheme really is in play: the bf16 reference's K/V differ by far more than the bound
    assert rel(prefill[L - 1][1], g["value_cache"][L - 1]) > 1e-2
    assert len(lat) == len(olat)
    for a, b in zip(lat, olat):
        e = rel(a, b)
        print(f"latents {e:.3g}")
        assert a.shape == b.shape and a.dtype == torch.float32 and e < 2e-2, e
    _tokens_match(toks, otoks, ologits, "tiny_d128 mxfp4 load mode")

    # unchanged refusals on a quantised engine
    eng = model.language_model.engine()
    with pytest.raises(NotImplementedError):
        eng.refresh()
    with pytest.raises(NotImplementedError):
        eng.fp8_weights()
    model.gen_weight_quant = "fp8"
    with pytest.raises(NotImplementedError):
        model.generate_image(past_key_values=cache, **cfg_kwargs("cfg_text", new_cache(cfg), g["cfg_inputs"]), **g["gen_kwargs"], **g["latent_inputs"])
    model.gen_weight_quant = None
    with pytest.raises(Exception):
        model.state_dict()


def test_mxfp4_load_mode_refuses_row_lengths_off_the_k_step_before_switching(monkeypatch):
    """hidden 128 / head_dim 32 (padded attention width 256) / intermediate 256 pass; TINY with hidden 192 does not: refused by name, nothing switched
    or released -- the contract of the "int8" refusal (tests/test_host_logic_cpu.py)."""
    install(monkeypatch)
    from bagel_amd.modeling.bagel.qwen2_navit import MoTEngine, mxfp4_refusal
    cfg = dict(TINY, name="tiny_h192", llm=dict(TINY["llm"], hidden_size=192, intermediate_size=320))
    from bagel_amd.factory import build_bagel
    model = build_bagel(cfg, device="cpu", with_vae=False)[0].to(torch.bfloat16).eval()          # (random weights: only the geometry matters)
    assert mxfp4_refusal(model.language_model.model.config)
    with pytest.raises(NotImplementedError, match="multiple of 128"):
        model.quantize_language_model("mxfp4")
    assert getattr(model.language_model, "weight_store", None) is None, "a refused mode must not leave the model half-switched"
    assert all(p.numel() > 0 for n, p in model.language_model.model.layers.named_parameters() if "proj" in n and n.endswith("weight"))
    with pytest.raises(NotImplementedError, match="multiple of 128"):
        MoTEngine(model.language_model.model, model.language_model.lm_head, weight_store="mxfp4")
    with pytest.raises(NotImplementedError):
        model.quantize_language_model("fp4")
    assert getattr(model.language_model, "weight_store", None) is None
    tok = StubTokenizer(cfg["llm"]["vocab_size"])
    gi, _, _ = model.prepare_prompts([0], [0], ["a small red cube"], tok, NEW_TOKEN_IDS_TINY)
    model.forward_cache_update_text(new_cache(cfg), **gi)          # still a working bf16 model
