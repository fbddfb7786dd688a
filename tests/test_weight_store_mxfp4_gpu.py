"""GPU: the whole-model load mode ``quantize_language_model("mxfp4")`` on the real kernels (bagel_gemm_w4_bf16 for prefill and denoise forwards,
bagel_gemv_w4_bf16 for the decode, one stored copy of the codes) against the ORACLE with the MXFP4 scheme switched into all fourteen projections of
every decoder layer (oracle/mxfp4.py; the set-up of tests/test_weight_store_mxfp4_cpu.py).

Bounds.  Nobody had measured this path, so they are tied to yardsticks of the parent commit.  For prefill K/V per layer, first-step velocity and final latents
two errors are measured against the MXFP4 oracle: ``e_q`` = the product in "mxfp4" mode, ``e_b`` = the *bf16* product (the size of the scheme's own effect).
  * prefill K/V, first-step velocity: ``e_q <= 0.5 * e_b`` -- the form tests/test_decode_gpu.py uses for the MXFP4 decode step (an implementation no closer to its
    own restatement than an engine that ignores the scheme has shown nothing); where 0.5 * e_b falls below the bf16 bound of tests/test_model_gpu.py for that
    quantity (1e-2 K/V, 2e-2 velocity) the bf16 bound is the gate.
  * final latents (4 Euler steps, CFG 4.0): the activation quantiser and its noise source are the FP8 option's (bf16-level GPU / CPU differences flip e4m3
    codes; tests/test_fp8_gpu.py measured 4.3e-2 on this model and request and froze 8e-2): ``e_q <= 8e-2`` and ``e_q < e_b``.
Every figure is printed before it is asserted.  End-to-end parity at 7B width rests on tests/test_gemm_w4_gpu.py's 7B shapes plus this tiny-model chain: the
7B-width test below checks finiteness, memory and the decode identity only (no MXFP4 oracle fixture at that width is committed)."""
import copy
import functools

import pytest
import torch

from oracle import bagel_oracle as O
from oracle.configs import TINY_D128, NEW_TOKEN_IDS_TINY, StubTokenizer
from tests.test_model_gpu import cfg_kwargs, new_cache, rel_l2
from tests.test_weight_store_mxfp4_cpu import all_projection_ptrs
from tests.util_models import _product, oracle_weights, product_model

pytestmark = pytest.mark.gpu


def _golden(name):
    return torch.load(__file__.rsplit("/", 1)[0] + f"/golden/{name}.pt", weights_only=False)


@functools.lru_cache(maxsize=1)
def _oracle_mxfp4():
    """Prefill K/V per layer, first-step velocity and final latents of the oracle with the scheme in all 14 x L projections."""
    from oracle import packers as P
    cfg = TINY_D128
    g = _golden("tiny_d128_t2i")
    W, _ = oracle_weights(cfg)
    L = cfg["llm"]["num_hidden_layers"]
    tok = StubTokenizer(cfg["llm"]["vocab_size"])
    gi, _, _ = P.prepare_prompts([0, 0], [0, 0], g["prompts"], tok, NEW_TOKEN_IDS_TINY)
    ci = g["cfg_inputs"]

    def cfgd():
        return dict(cache=O.OracleCache(L), position_ids=ci["cfg_packed_position_ids"], query_indexes=ci["cfg_packed_query_indexes"],
                    key_values_lens=ci["cfg_key_values_lens"], key_value_indexes=ci["cfg_packed_key_value_indexes"])
    # the oracle caches quantised weights by (data_ptr, version): entries of weight tensors an earlier test has since freed must not be found again
    O.linear.__dict__.pop("_mx", None)
    O.MXFP4_WEIGHT_PTRS = all_projection_ptrs(W)
    try:
        assert len(O.MXFP4_WEIGHT_PTRS) == 14 * L
        oc = O.forward_cache_update_text(W, cfg, O.OracleCache(L), **gi)
        kv = [(oc.key_cache[i].clone(), oc.value_cache[i].clone()) for i in range(L)]
        li = g["latent_inputs"]
        ts, _ = O.flow_schedule(5, 3.0)
        timestep = torch.tensor([ts[0]] * li["packed_init_noises"].shape[0])
        v0 = O.forward_flow(W, cfg, li["packed_init_noises"], timestep, li, oc, cfgd(), None, 4.0, 1.0, 0.0, "global")
        lat = O.generate_image(W, cfg, li, oc, cfg_text=cfgd(), **g["gen_kwargs"])
    finally:
        O.MXFP4_WEIGHT_PTRS = set()
        O.linear.__dict__.pop("_mx", None)
    return kv, v0, list(lat)


def _run(model, cfg, g):
    tok = StubTokenizer(cfg["llm"]["vocab_size"])
    L = cfg["llm"]["num_hidden_layers"]
    gi, newlens, newrope = model.prepare_prompts([0, 0], [0, 0], g["prompts"], tok, NEW_TOKEN_IDS_TINY)
    cache = model.forward_cache_update_text(new_cache(cfg), **gi)
    kv = [(cache.key_cache[i].clone(), cache.value_cache[i].clone()) for i in range(L)]
    li = dict(g["latent_inputs"])
    x = li.pop("packed_init_noises")
    ts, _ = model.flow_schedule(5, 3.0)
    v0 = model._forward_flow(x_t=x, timestep=torch.tensor([ts[0]] * x.shape[0]), past_key_values=cache, cfg_text_scale=4.0, cfg_renorm_type="global",
                             **cfg_kwargs("cfg_text", new_cache(cfg), g["cfg_inputs"]), **li)
    lat = model.generate_image(past_key_values=cache, **cfg_kwargs("cfg_text", new_cache(cfg), g["cfg_inputs"]), **g["gen_kwargs"], **g["latent_inputs"])
    st = model.prepare_start_tokens(newlens, newrope, NEW_TOKEN_IDS_TINY)
    return cache, kv, v0, list(lat), st


def test_mxfp4_load_mode_matches_its_restatement():
    cfg = TINY_D128
    g = _golden("tiny_d128_t2i")
    okv, ov0, olat = _oracle_mxfp4()
    bm, _ = product_model(cfg)                                     # the shared bf16 model: read only
    qm, _ = _product.__wrapped__(cfg["name"])                      # a fresh one to quantise
    full = sum(p.numel() * 2 for n, p in qm.language_model.model.layers.named_parameters() if "proj" in n and n.endswith("weight"))
    before = torch.cuda.memory_allocated()
    resident = qm.quantize_language_model("mxfp4", release_bf16=True)
    assert resident < 0.28 * full
    assert torch.cuda.memory_allocated() < before, "releasing the bf16 projection weights must free more than the codes take"
    qcache, qkv, qv0, qlat, st = _run(qm, cfg, g)
    _, bkv, bv0, blat, _ = _run(bm, cfg, g)
    for i, ((qk, qv), (bk, bv), (ok, ov)) in enumerate(zip(qkv, bkv, okv)):
        for what, q_, b_, o_ in (("K", qk, bk, ok), ("V", qv, bv, ov)):
            e_q, e_b = rel_l2(q_, o_), rel_l2(b_, o_)
            gate = max(0.5 * e_b, 1e-2)
            print(f"prefill {what} layer {i}: e_q {e_q:.3g}  e_b {e_b:.3g}  gate {gate:.3g}")
            assert e_q <= gate, f"prefill {what} layer {i}: e_q {e_q:.3g} > {gate:.3g} (e_b {e_b:.3g})"
    e_q, e_b = rel_l2(qv0, ov0), rel_l2(bv0, ov0)
    gate = max(0.5 * e_b, 2e-2)
    print(f"first-step velocity: e_q {e_q:.3g}  e_b {e_b:.3g}  gate {gate:.3g}")
    assert e_q <= gate, f"first-step velocity: e_q {e_q:.3g} > {gate:.3g} (e_b {e_b:.3g})"
    for a, b, o in zip(qlat, blat, olat):
        e_q, e_b = rel_l2(a, o), rel_l2(b, o)
        print(f"final latents: e_q {e_q:.3g}  e_b {e_b:.3g}")
        assert torch.isfinite(a).all() and e_q <= 8e-2 and e_q < e_b, f"final latents: e_q {e_q:.3g} (band 8e-2), e_b {e_b:.3g}"

    # decode in the mode: graph replay == eager bit for bit; the same tokens as weight_quant="mxfp4" on the bf16 engine from the same cache
    n = 8
    a = qm.generate_text(past_key_values=copy.deepcopy(qcache), max_length=n, do_sample=False, end_token_id=None, use_graph=True, **st)
    sess = qm._last_decode_session
    assert sess.weight_quant == "mxfp4" and sess.graph is not None
    b = qm.generate_text(past_key_values=copy.deepcopy(qcache), max_length=n, do_sample=False, end_token_id=None, use_graph=False, **st)
    assert torch.equal(a, b), "graph replay differs from the eager decode"
    c = bm.generate_text(past_key_values=copy.deepcopy(qcache), max_length=n, do_sample=False, end_token_id=None, weight_quant="mxfp4", **st)
    assert torch.equal(a, c), "the mode's decode differs from weight_quant='mxfp4' on a bf16 engine (same kernels, same codes)"
    with pytest.raises(NotImplementedError):
        qm.language_model.engine().refresh()


def _peak_of_mode(kind, cfg, g):
    """Peak device bytes above the start of one model's life: build, switch to ``kind``, one prefill + one denoise step."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    model, _ = _product.__wrapped__(cfg["name"])
    model.quantize_language_model(kind, release_bf16=True)
    tok = StubTokenizer(cfg["llm"]["vocab_size"])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    gi, _, _ = model.prepare_prompts([0, 0], [0, 0], g["prompts"], tok, NEW_TOKEN_IDS_TINY)
    cache = model.forward_cache_update_text(new_cache(cfg), **gi)
    li = dict(g["latent_inputs"])
    x = li.pop("packed_init_noises")
    ts, _ = model.flow_schedule(5, 3.0)
    model._forward_flow(x_t=x, timestep=torch.tensor([ts[0]] * x.shape[0]), past_key_values=cache, cfg_text_scale=4.0, cfg_renorm_type="global",
                        **cfg_kwargs("cfg_text", new_cache(cfg), g["cfg_inputs"]), **li)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del model, cache
    return peak


def test_mxfp4_load_mode_peak_is_below_nf4():
    """No scratch sets: codes of about the same size, and nothing de-quantised beside them.  One un-measured pass comes first: the first forward of a
    process leaves process-wide allocations behind (attention work lists, split-K partial buffers, RoPE tables) that would be charged to whichever
    mode runs first."""
    cfg = TINY_D128
    g = _golden("tiny_d128_t2i")
    _peak_of_mode("nf4", cfg, g)
    _peak_of_mode("mxfp4", cfg, g)
    p4 = _peak_of_mode("mxfp4", cfg, g)
    pn = _peak_of_mode("nf4", cfg, g)
    print(f"peak over prefill + one denoise step: mxfp4 {p4} B, nf4 {pn} B")
    assert p4 < pn


def test_mxfp4_load_mode_at_7b_width(golden):
    """BAGEL-7B-MoT WIDTH (hidden 3584, intermediate 18944, 28 / 4 heads of 128, 2 MoT layers), the 512^2 text->image request of tests/golden/wide7b_options.pt
    (4 timesteps, CFG 4.0) + 6 greedy tokens: finite latents that differ from bf16 by the scheme's size, the decode identity, the resident size."""
    from oracle.configs import WIDE7B as cfg
    from tests.test_wide_gpu import _options_context, _wide_model
    g = golden("wide7b_options")
    qm, bm = _wide_model(), _wide_model()
    full = sum(p.numel() * 2 for n, p in bm.language_model.model.layers.named_parameters() if "proj" in n and n.endswith("weight"))
    before = torch.cuda.memory_allocated()
    resident = qm.quantize_language_model("mxfp4")
    assert resident < 0.28 * full
    assert torch.cuda.memory_allocated() < before
    with pytest.raises(RuntimeError, match="release_bf16"):
        qm.state_dict()
    kw, c = g["fp8"]["gen_kwargs"], g["cfg_inputs"]
    cache = _options_context(qm, cfg, g)
    lat = qm.generate_image(past_key_values=cache, **cfg_kwargs("cfg_text", new_cache(cfg), c), **kw, **g["latent_inputs"])
    blat = bm.generate_image(past_key_values=_options_context(bm, cfg, g), **cfg_kwargs("cfg_text", new_cache(cfg), c), **kw, **g["latent_inputs"])
    for a, b in zip(lat, blat):
        e = rel_l2(a, b)
        print(f"7B width: latents in the mode vs bf16 {e:.3g}")
        assert torch.isfinite(a).all() and 0 < e < 0.5
    st = qm.prepare_start_tokens([cache.seq_lens], [cache.seq_lens], NEW_TOKEN_IDS_TINY)
    a = qm.generate_text(past_key_values=copy.deepcopy(cache), max_length=6, do_sample=False, end_token_id=None, use_graph=True, **st)
    assert qm._last_decode_session.weight_quant == "mxfp4" and qm._last_decode_session.graph is not None
    b = qm.generate_text(past_key_values=copy.deepcopy(cache), max_length=6, do_sample=False, end_token_id=None, use_graph=False, **st)
    c2 = bm.generate_text(past_key_values=copy.deepcopy(cache), max_length=6, do_sample=False, end_token_id=None, weight_quant="mxfp4", **st)
    assert torch.equal(a, b) and torch.equal(a, c2)
    print(f"whole-model mxfp4 at 7B width: resident {resident / 1e6:.0f} MB of {full / 1e6:.0f} MB")
