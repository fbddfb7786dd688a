"""CPU: the routing of a batched decode step on MXFP4 weights (modeling/bagel/decode.py) on the torch stand-ins of tests/mock_ops.py: more than four requests
quantise their activation rows with a launch of their own (rmsnorm_fp8 in front of qkv and gate/up, quantize_rows_fp8 in front of o and down) into buffers the
session owns; 5..32 requests then take ``ops.gemv_mb_w4``, more than 32 (or a refused shape, or BAGEL_GEMV_MB_W4=0) ``ops.gemm_w4``; the lm_head stays bf16.
The stand-in for the stream is oracle/mxfp4.py::gemv_w4's product on already quantised rows (as tests/test_weight_store_mxfp4_cpu.py does for gemm_w4), and
the step is compared with the ORACLE's decode step with the MXFP4 scheme switched into the same seven linears per layer.  The gate on the first-step logits is
the one this comparison already has (tests/test_decode_gpu.py::test_generate_text_mxfp4_weights_option: an e4m3 activation code next to a rounding boundary
flips on a bf16-level difference of its input, so ``e < 8e-2`` -- the band frozen for the FP8 quantiser -- and ``e < 0.5 * e_bf16``, half the distance of the
*bf16* product to the same restatement: an implementation no closer to its restatement than one that ignores the scheme has shown nothing); the greedy ids
follow the token rule of tests/test_host_logic_cpu.py::test_decode_mxfp4_weights_host_path_matches_oracle."""
import os

import pytest
import torch

from oracle import bagel_oracle as O
from oracle.configs import TINY_D128, NEW_TOKEN_IDS_TINY, StubTokenizer
from tests import mock_ops
from tests.test_host_logic_cpu import _tokens_match, cpu_model, new_cache, rel
from tests.test_weight_store_mxfp4_cpu import gemm_w4 as gemm_w4_stand_in
from tests.util_models import oracle_weights


def install(monkeypatch, calls):
    from bagel_amd import ops
    mock_ops.install(monkeypatch)

    def gemv_mb_w4(Aq, sa, Wq, Ws, C, *, bias=None, residual=None, epilogue=0, M=None, workspace=None):
        assert 1 <= M <= 32 and Aq.dtype == torch.uint8 and sa.dtype == torch.float32
        calls.append(("gemv_mb_w4", M, Wq.shape[0], Wq.shape[1] * 2, epilogue))
        return gemm_w4_stand_in(Aq, sa, Wq, Ws, C, bias=bias, M=M, residual=residual, epilogue=epilogue)

    def gemm_w4(Aq, sa, Wq, Ws, C, *, bias=None, rows=None, M=None, residual=None, epilogue=0):
        calls.append(("gemm_w4", M, Wq.shape[0], Wq.shape[1] * 2, epilogue))
        return gemm_w4_stand_in(Aq, sa, Wq, Ws, C, bias=bias, rows=rows, M=M, residual=residual, epilogue=epilogue)

    def gemv_mb_w4_supported(Aq, Wq, Ws, C, bias, residual, epilogue, M=None):
        return os.environ.get("BAGEL_GEMV_MB_W4", "1") != "0" and 1 <= M <= 32 and not (epilogue == 3 and (bias is not None or residual is not None))

    def gemv_w4(*a, **kw):
        calls.append(("gemv_w4", kw.get("M")))
        return mock_ops.gemv_w4(*a, **kw)
    monkeypatch.setattr(ops, "gemv_mb_w4", gemv_mb_w4, raising=False)
    monkeypatch.setattr(ops, "gemm_w4", gemm_w4)
    monkeypatch.setattr(ops, "gemv_mb_w4_supported", gemv_mb_w4_supported, raising=False)
    monkeypatch.setattr(ops, "mb_w4_workspace_floats", lambda N, K: 0, raising=False)
    monkeypatch.setattr(ops, "gemv_w4", gemv_w4)


def prompts_for(B):
    return [("word " * (1 + i % 7)).strip() + f" {i}" for i in range(B)]


@pytest.mark.parametrize("B,knob,route", [(5, None, "gemv_mb_w4"), (40, None, "gemm_w4"), (5, "0", "gemm_w4"), (4, None, "gemv_w4")])
def test_batched_mxfp4_decode_route_and_oracle(monkeypatch, B, knob, route):
    calls = []
    install(monkeypatch, calls)
    monkeypatch.setenv("BAGEL_DECODE_GRAPH", "0")
    if knob is not None:
        monkeypatch.setenv("BAGEL_GEMV_MB_W4", knob)
    else:
        monkeypatch.delenv("BAGEL_GEMV_MB_W4", raising=False)
    cfg = TINY_D128
    model = cpu_model(cfg)
    W, _ = oracle_weights(cfg)
    L = cfg["llm"]["num_hidden_layers"]
    tok = StubTokenizer(cfg["llm"]["vocab_size"])
    pi, l2, r2 = model.prepare_prompts([0] * B, [0] * B, prompts_for(B), tok, NEW_TOKEN_IDS_TINY)
    assert len(set(l2)) > 1, "the requests have unequal prompt lengths"
    cache = model.forward_cache_update_text(new_cache(cfg), **pi)
    oc = O.forward_cache_update_text(W, cfg, O.OracleCache(L), **pi)
    si = model.prepare_start_tokens(l2, r2, NEW_TOKEN_IDS_TINY)
    n = 2
    O.linear.__dict__.pop("_mx", None)
    O.MXFP4_WEIGHT_PTRS = O.mxfp4_decode_weight_ptrs(W)
    try:
        otoks, ologits = O.generate_text(W, cfg, oc, si["packed_key_value_indexes"], si["key_values_lens"], si["packed_start_tokens"],
                                         si["packed_query_position_ids"], n, return_logits=True)
    finally:
        O.MXFP4_WEIGHT_PTRS = set()
        O.linear.__dict__.pop("_mx", None)
    model.generate_text(past_key_values=model.forward_cache_update_text(new_cache(cfg), **pi), max_length=1, do_sample=False, end_token_id=None, use_graph=False, **si)
    ol = torch.as_tensor(ologits[0]).float()
    e_bf16 = rel(model._last_decode_session.logits.float(), ol.reshape(model._last_decode_session.logits.shape))
    del calls[:]
    one = model.generate_text(past_key_values=cache, max_length=1, do_sample=False, end_token_id=None, use_graph=False, weight_quant="mxfp4", **si)
    sess = model._last_decode_session
    assert sess.weight_quant == "mxfp4" and one.shape == (1, B)
    # the route: four projections per layer, all on the same kernel, with the epilogues of the layer; nothing else touched the codes
    assert {c[0] for c in calls} == {route}, sorted({c[0] for c in calls})
    assert len(calls) == 4 * L
    if route != "gemv_w4":
        assert all(c[1] == B for c in calls) and [c[4] for c in calls[:4]] == [0, 0, 3, 0]
        assert sess.aq8.dtype == torch.uint8 and sess.aq8.shape[0] == B and sess.sa.shape == (B,)
    e = rel(sess.logits.float(), ol.reshape(sess.logits.shape))
    print(f"B={B} route {route}: first-step logits vs the oracle's MXFP4 decode step: rel_l2 {e:.3g} (the bf16 product vs the same restatement: {e_bf16:.3g})")
    assert e < 8e-2 and e < 0.5 * e_bf16, (e, e_bf16)
    # ... and a second step through the same session state (KV append, positions): greedy ids up to the oracle's first near tie
    cache2 = model.forward_cache_update_text(new_cache(cfg), **pi)
    toks = model.generate_text(past_key_values=cache2, max_length=n, do_sample=False, end_token_id=None, use_graph=False, weight_quant="mxfp4", **si)
    _tokens_match(toks, otoks, ologits, f"tiny_d128 mxfp4 B={B}")
    assert cache2.lens(0) == [x + n for x in l2]
