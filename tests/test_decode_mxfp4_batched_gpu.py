"""GPU: batched text decode on MXFP4 weights (modeling/bagel/decode.py): more than four requests per weight pass -- 5..32 on the weight stream of
csrc/gemv_mb_w4.hip behind a quantiser launch, more than 32 (and BAGEL_GEMV_MB_W4=0) on the large-M kernel -- through ``generate_text(weight_quant="mxfp4")``,
the model-level switch and the whole-model load mode; the identities tests/test_weight_store_mxfp4_gpu.py checks at batch 1.  The first-step logits are pinned
to the ORACLE's decode step with the MXFP4 scheme switched into the same seven linears per layer (bf16 prefill on both sides), per request row, with the gate
of tests/test_decode_gpu.py::test_generate_text_mxfp4_weights_option: ``e < 8e-2`` and ``e < 0.5 * e_bf16`` (e_bf16 = the bf16 product's distance to the same
restatement).  Every figure is printed before it is asserted."""
import copy
import functools

import pytest
import torch

from oracle import bagel_oracle as O
from oracle.configs import TINY_D128 as cfg, NEW_TOKEN_IDS_TINY, StubTokenizer
from tests.test_decode_gpu import _context
from tests.util_models import _product, oracle_weights, product_model

pytestmark = pytest.mark.gpu


def prompts_for(B):
    return [("word " * (1 + i % 7)).strip() + f" {i}" for i in range(B)]


def rows_rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm(dim=-1) / b.norm(dim=-1).clamp_min(1e-30))


@functools.lru_cache(maxsize=None)
def stream_run(B):
    """One shared run per batch size on the shared bf16 model: context, 8 graph-replayed tokens, the first-step logits of the mxfp4 and the bf16 step."""
    model, _ = product_model(cfg)
    cache, lens, ropes, start = _context(model, cfg, prompts_for(B))
    assert len(set(lens)) > 1
    model.generate_text(past_key_values=copy.deepcopy(cache), max_length=1, end_token_id=None, weight_quant="mxfp4", **start)
    q1 = model._last_decode_session.logits.float().cpu().clone()
    model.generate_text(past_key_values=copy.deepcopy(cache), max_length=1, end_token_id=None, **start)
    b1 = model._last_decode_session.logits.float().cpu().clone()
    c = copy.deepcopy(cache)
    toks = model.generate_text(past_key_values=c, max_length=8, end_token_id=None, weight_quant="mxfp4", use_graph=True, **start)
    sess = model._last_decode_session
    return dict(model=model, cache=cache, lens=lens, start=start, q1=q1, b1=b1, toks=toks, graph=sess.graph is not None, graph_error=sess.graph_error,
                grown=c.seq_lens - cache.seq_lens, cache_after=c)


@pytest.mark.parametrize("B", [5, 20])
def test_batched_mxfp4_decode_identities(B):
    r = stream_run(B)
    model, cache, start, a = r["model"], r["cache"], r["start"], r["toks"]
    assert r["graph"], f"hipGraph capture failed: {r['graph_error']}"
    assert a.shape == (8, B) and r["grown"] == 8 * B, "the caller's cache grows by one row per request and token"
    c_eager = copy.deepcopy(cache)
    b = model.generate_text(past_key_values=c_eager, max_length=8, end_token_id=None, weight_quant="mxfp4", use_graph=False, **start)
    assert torch.equal(a, b), "graph replay differs from eager stepping"
    for i in range(cfg["llm"]["num_hidden_layers"]):
        assert torch.equal(r["cache_after"].key_cache[i], c_eager.key_cache[i]) and torch.equal(r["cache_after"].value_cache[i], c_eager.value_cache[i])
    model.decode_weight_quant = "mxfp4"                              # the model-level switch
    try:
        c = model.generate_text(past_key_values=copy.deepcopy(cache), max_length=8, end_token_id=None, **start)
        assert model._last_decode_session.weight_quant == "mxfp4"
    finally:
        model.decode_weight_quant = None
    assert torch.equal(a, c), "decode_weight_quant='mxfp4' differs from weight_quant='mxfp4'"
    qm, _ = _product.__wrapped__(cfg["name"])                        # a fresh model in the whole-model load mode, run from the same cache
    qm.quantize_language_model("mxfp4", release_bf16=True)
    d = qm.generate_text(past_key_values=copy.deepcopy(cache), max_length=8, end_token_id=None, use_graph=True, **start)
    sess = qm._last_decode_session
    assert sess.weight_quant == "mxfp4" and sess.graph is not None
    assert torch.equal(a, d), "the load mode's decode differs from weight_quant='mxfp4' on a bf16 engine (same kernels, same codes)"


def test_first_step_logits_against_the_oracle():
    B = 5
    r = stream_run(B)
    model, start = r["model"], r["start"]
    W, _ = oracle_weights(cfg)
    L = cfg["llm"]["num_hidden_layers"]
    gi, _, _ = model.prepare_prompts([0] * B, [0] * B, prompts_for(B), StubTokenizer(cfg["llm"]["vocab_size"]), NEW_TOKEN_IDS_TINY)
    oc = O.forward_cache_update_text(W, cfg, O.OracleCache(L), **gi)
    O.linear.__dict__.pop("_mx", None)
    O.MXFP4_WEIGHT_PTRS = O.mxfp4_decode_weight_ptrs(W)
    try:
        st = {k: torch.as_tensor(v).cpu() for k, v in start.items()}
        _, ologits = O.generate_text(W, cfg, oc, st["packed_key_value_indexes"], st["key_values_lens"], st["packed_start_tokens"],
                                     st["packed_query_position_ids"], 1, return_logits=True)
    finally:
        O.MXFP4_WEIGHT_PTRS = set()
        O.linear.__dict__.pop("_mx", None)
    ol = torch.as_tensor(ologits[0]).float().reshape(r["q1"].shape)
    e, e_bf16 = rows_rel(r["q1"], ol), rows_rel(r["b1"], ol)
    for m in range(B):
        print(f"request {m}: mxfp4 step vs its restatement rel_l2 {e[m].item():.3g}  (bf16 step vs the same restatement {e_bf16[m].item():.3g})")
    for m in range(B):
        assert e[m] < 8e-2 and e[m] < 0.5 * e_bf16[m], f"request {m}: {e[m].item():.3g} (bf16: {e_bf16[m].item():.3g})"


@pytest.mark.parametrize("B,knob", [(40, None), (20, "0")], ids=["forty", "knob_off_twenty"])
def test_gemm_w4_fallback_routes(monkeypatch, B, knob):
    """More than 32 requests, and 5..32 with BAGEL_GEMV_MB_W4=0, run on ops.gemm_w4: graph == eager, and their first-step logits on the requests shared with
    the 20-request stream run (the prompts are a prefix of one list) sit within the gate of the oracle comparison."""
    from bagel_amd import ops
    ref = stream_run(20)
    if knob is not None:
        monkeypatch.setenv("BAGEL_GEMV_MB_W4", knob)
    seen = []
    real_gemm_w4, real_stream = ops.gemm_w4, ops.gemv_mb_w4
    monkeypatch.setattr(ops, "gemm_w4", lambda *a, **k: (seen.append("gemm_w4"), real_gemm_w4(*a, **k))[1])
    monkeypatch.setattr(ops, "gemv_mb_w4", lambda *a, **k: (seen.append("gemv_mb_w4"), real_stream(*a, **k))[1])
    model, _ = product_model(cfg)
    cache, lens, ropes, start = _context(model, cfg, prompts_for(B))
    model.generate_text(past_key_values=copy.deepcopy(cache), max_length=1, end_token_id=None, weight_quant="mxfp4", use_graph=False, **start)
    q1 = model._last_decode_session.logits.float().cpu().clone()
    assert set(seen) == {"gemm_w4"}, set(seen)
    a = model.generate_text(past_key_values=copy.deepcopy(cache), max_length=8, end_token_id=None, weight_quant="mxfp4", use_graph=True, **start)
    sess = model._last_decode_session
    assert sess.graph is not None, f"hipGraph capture failed: {sess.graph_error}"
    b = model.generate_text(past_key_values=copy.deepcopy(cache), max_length=8, end_token_id=None, weight_quant="mxfp4", use_graph=False, **start)
    assert a.shape == (8, B) and torch.equal(a, b), "graph replay differs from eager stepping"
    e, e_bf16 = rows_rel(q1[:20], ref["q1"]), rows_rel(ref["b1"], ref["q1"])
    print(f"B={B} knob={knob}: fallback vs stream, first-step logits per shared request: worst rel_l2 {e.max().item():.3g} (bf16 vs stream: least {e_bf16.min().item():.3g})")
    assert (e < 8e-2).all() and (e < 0.5 * e_bf16).all(), (e.tolist(), e_bf16.tolist())
