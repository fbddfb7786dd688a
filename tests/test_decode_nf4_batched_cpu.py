"""CPU: the routing of a batched decode step on NF4 weights (modeling/bagel/decode.py) on the torch stand-ins of tests/mock_ops.py: 5..32 requests run
``ops.rmsnorm`` into the session's ``h`` buffer where a norm precedes the projection (qkv, gate/up) and then ``ops.gemv_mb_nf4`` -- one pass over the codes for
all rows; up to 4 requests, more than 32, a refused shape or BAGEL_GEMV_MB_NF4=0 keep the unchanged ``ops.gemv_nf4`` call with the norm fused; the lm_head stays
bf16.  The stand-in for the stream is mock_ops.gemv on oracle/nf4.py::dequantize_nf4 (the bf16 weight the kernel builds in registers), and the step is compared
with the ORACLE's decode step with the NF4 scheme switched into the same seven linears per layer.  The gate on the first-step logits is the one this comparison
already has (tests/test_nf4_gpu.py::test_generate_text_nf4_weights_option: identical codes on both sides, bf16 activations: ``e < 2e-2`` and
``e < 0.5 * e_bf16``, half the distance of the *bf16* product to the same restatement); the greedy ids follow the token rule of
tests/test_host_logic_cpu.py::test_decode_nf4_weights_host_path_matches_oracle."""
import os

import pytest
import torch

from oracle import bagel_oracle as O
from oracle import nf4 as NF
from oracle.configs import TINY_D128, NEW_TOKEN_IDS_TINY, StubTokenizer
from tests import mock_ops
from tests.test_host_logic_cpu import _tokens_match, cpu_model, new_cache, rel
from tests.util_models import oracle_weights


def install(monkeypatch, calls):
    from bagel_amd import ops
    mock_ops.install(monkeypatch)

    def gemv_mb_nf4(A, Wq, absmax, C, *, bias=None, residual=None, epilogue=0, M=None, workspace=None):
        assert 1 <= M <= 32 and A.dtype == torch.bfloat16 and absmax.shape == (Wq.shape[0], Wq.shape[1] * 2 // 64)
        calls.append(("gemv_mb_nf4", M, Wq.shape[0], Wq.shape[1] * 2, epilogue, A.data_ptr()))
        return mock_ops.gemv(A, NF.dequantize_nf4(Wq, absmax), C, bias=bias, residual=residual, epilogue=epilogue, M=M)

    def gemv_mb_nf4_supported(A, Wq, absmax, C, bias, residual, epilogue, M=None):
        K = Wq.shape[1] * 2
        return (os.environ.get("BAGEL_GEMV_MB_NF4", "1") != "0" and 1 <= M <= 32 and K % 128 == 0 and Wq.shape[0] % (32 if epilogue == 3 else 16) == 0
                and not (epilogue == 3 and (bias is not None or residual is not None)))

    def gemv_nf4(A, Wq, absmax, C, **kw):
        calls.append(("gemv_nf4", kw.get("M"), Wq.shape[0], Wq.shape[1] * 2, kw.get("epilogue", 0), kw.get("norm_w") is not None))
        return mock_ops.gemv_nf4(A, Wq, absmax, C, **kw)

    def rmsnorm(x, w0, out, eps, *a, **kw):
        calls.append(("rmsnorm", x.shape[0], out.data_ptr()))
        return mock_ops.rmsnorm(x, w0, out, eps, *a, **kw)
    monkeypatch.setattr(ops, "gemv_mb_nf4", gemv_mb_nf4, raising=False)
    monkeypatch.setattr(ops, "gemv_mb_nf4_supported", gemv_mb_nf4_supported, raising=False)
    monkeypatch.setattr(ops, "mb_nf4_workspace_floats", lambda N, K: 0, raising=False)
    monkeypatch.setattr(ops, "gemv_nf4", gemv_nf4)
    monkeypatch.setattr(ops, "rmsnorm", rmsnorm)


def prompts_for(B):
    return [("word " * (1 + i % 7)).strip() + f" {i}" for i in range(B)]


@pytest.mark.parametrize("B,knob,route", [(5, None, "gemv_mb_nf4"), (32, None, "gemv_mb_nf4"), (40, None, "gemv_nf4"), (5, "0", "gemv_nf4"), (4, None, "gemv_nf4")])
def test_batched_nf4_decode_route_and_oracle(monkeypatch, B, knob, route):
    calls = []
    install(monkeypatch, calls)
    monkeypatch.setenv("BAGEL_DECODE_GRAPH", "0")
    if knob is not None:
        monkeypatch.setenv("BAGEL_GEMV_MB_NF4", knob)
    else:
        monkeypatch.delenv("BAGEL_GEMV_MB_NF4", raising=False)
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
    O.NF4_WEIGHT_PTRS = O.mxfp4_decode_weight_ptrs(W)          # the same seven linears per layer
    try:
        otoks, ologits = O.generate_text(W, cfg, oc, si["packed_key_value_indexes"], si["key_values_lens"], si["packed_start_tokens"],
                                         si["packed_query_position_ids"], n, return_logits=True)
    finally:
        O.NF4_WEIGHT_PTRS = set()
    model.generate_text(past_key_values=model.forward_cache_update_text(new_cache(cfg), **pi), max_length=1, do_sample=False, end_token_id=None, use_graph=False, **si)
    ol = torch.as_tensor(ologits[0]).float()
    e_bf16 = rel(model._last_decode_session.logits.float(), ol.reshape(model._last_decode_session.logits.shape))
    del calls[:]
    one = model.generate_text(past_key_values=cache, max_length=1, do_sample=False, end_token_id=None, use_graph=False, weight_quant="nf4", **si)
    sess = model._last_decode_session
    assert sess.weight_quant == "nf4" and one.shape == (1, B)
    # the route: four projections per layer, all on the same op, with the epilogues of the layer; nothing else touched the codes
    projs = [c for c in calls if c[0] != "rmsnorm"]
    assert {c[0] for c in projs} == {route}, sorted({c[0] for c in projs})
    assert len(projs) == 4 * L
    assert all(c[1] == B for c in projs) and [c[4] for c in projs[:4]] == [0, 0, 3, 0]
    # the stream takes its norm as a launch of its own in front of qkv and gate/up, into the session's h buffer, which the projection then reads; the old route
    # keeps the norm fused (the final norm in front of the bf16 lm_head comes after the last projection and is not this route's business)
    body = calls[:max(i for i, c in enumerate(calls) if c[0] == route) + 1]
    if route == "gemv_mb_nf4":
        names = [c[0] for c in body]
        assert names == ["rmsnorm", route, route, "rmsnorm", route, route] * L, names[:6]
        norms = [c for c in body if c[0] == "rmsnorm"]
        assert all(c[1] == B and c[2] == sess.h.data_ptr() for c in norms)
        assert all(projs[4 * li + j][5] == sess.h.data_ptr() for li in range(L) for j in (0, 2))
        assert all(projs[4 * li + j][5] != sess.h.data_ptr() for li in range(L) for j in (1, 3))
    else:
        assert not [c for c in body if c[0] == "rmsnorm"]
        assert all(projs[4 * li + j][5] == (j in (0, 2)) for li in range(L) for j in range(4))
    e = rel(sess.logits.float(), ol.reshape(sess.logits.shape))
    print(f"B={B} route {route}: first-step logits vs the oracle's NF4 decode step: rel_l2 {e:.3g} (the bf16 product vs the same restatement: {e_bf16:.3g})")
    assert e < 2e-2 and e < 0.5 * e_bf16, (e, e_bf16)
    # ... and a second step through the same session state (KV append, positions): greedy ids up to the oracle's first near tie
    cache2 = model.forward_cache_update_text(new_cache(cfg), **pi)
    toks = model.generate_text(past_key_values=cache2, max_length=n, do_sample=False, end_token_id=None, use_graph=False, weight_quant="nf4", **si)
    _tokens_match(toks, otoks, ologits, f"tiny_d128 nf4 B={B}")
    assert cache2.lens(0) == [x + n for x in l2]
