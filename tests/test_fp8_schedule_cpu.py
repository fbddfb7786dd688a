"""CPU: WHEN the FP8 gen expert quantises the SwiGLU output with delayed scales (the rule of qwen2_navit.Fp8DelayedScales) across the schedules of a
denoise loop -- CFG interval switches, stream-batched and sequential CFG, TaylorSeer step skipping, the 3-stream edit form.

The product runs on the torch stand-ins of tests/mock_ops.py (built on oracle/fp8.py); every down-projection input of the gen expert is recorded as
(step, stream, layer, "exact" | "delayed", age), age = Euler steps since the same stream's rows at that layer were last quantised.  The oracle's
restatement (oracle/fp8.py DelayedScales) records the same trace from its own sequential forwards.  The two must agree, and no delayed scale may come
from rows older than the immediately preceding step."""
import copy

import pytest
import torch

from oracle.configs import TINY_D128, NEW_TOKEN_IDS_TINY, StubTokenizer
from tests import mock_ops
from tests.test_host_logic_cpu import cfg_kwargs, cpu_model, new_cache
from tests.util_models import oracle_weights


def _setup(model, cfg, sizes, streams):
    from oracle import bagel_oracle as O
    W, _ = oracle_weights(cfg)
    L = cfg["llm"]["num_hidden_layers"]
    tok = StubTokenizer(cfg["llm"]["vocab_size"])
    ids = NEW_TOKEN_IDS_TINY
    B = len(sizes)
    ctx = []
    for prompts in (["a small red cube on the table", "sky"][:B], ["cube", "a b"][:B], ["x y z w v", "hello world again"][:B])[:streams]:
        gi, lens, ropes = model.prepare_prompts([0] * B, [0] * B, prompts, tok, ids)
        ctx.append((model.forward_cache_update_text(new_cache(cfg), **gi), O.forward_cache_update_text(W, cfg, O.OracleCache(L), **gi), lens, ropes))
    torch.manual_seed(11)
    li = model.prepare_vae_latent(ctx[0][2], ctx[0][3], sizes, ids)
    kw, okw = {}, {}
    for tag, (c, oc, lens, ropes) in zip(("cfg_text", "cfg_img"), ctx[1:]):
        d = model.prepare_vae_latent_cfg(lens, ropes, sizes)
        kw.update(cfg_kwargs(tag, c, d))
        okw[tag] = dict(cache=oc, position_ids=d["cfg_packed_position_ids"], query_indexes=d["cfg_packed_query_indexes"],
                        key_values_lens=d["cfg_key_values_lens"], key_value_indexes=d["cfg_packed_key_value_indexes"])
    return W, li, ctx[0][0], ctx[0][1], kw, okw


def _product_trace(monkeypatch, model, M1, run):
    """Run ``run()`` and record every gen-expert down projection the product's engine launches (observed at the operator level)."""
    from bagel_amd import ops
    from bagel_amd.modeling.bagel import bagel as B
    eng = model.language_model.engine()
    trace, last, cur, states = [], {}, {"step": 0, "state": None, "S": 1}, []
    cls = B.Fp8DelayedScales
    monkeypatch.setattr(B, "Fp8DelayedScales", lambda *a, **k: states.append(cls(*a, **k)) or states[-1])     # generate_image's f8[0..3], in order
    model.step_hook = lambda i, x: cur.update(step=i)                       # called after Euler step i - 1: the next one is step i
    orig_forward, orig_gemm = eng.forward, ops.gemm_fp8

    def forward(seq, plan, *a, **k):
        st = k.get("fp8_state")
        cur.update(state=next((i for i, s in enumerate(states[-4:]) if s is st), None) if st is not None else None, S=plan.M // M1)
        return orig_forward(seq, plan, *a, **k)

    def gemm_fp8(Aq, sa, Wq, sw, C, **k):
        wd = {Q["wd"][0].data_ptr(): li for li, Q in enumerate(eng.fp8_weights())}
        li = wd.get(Wq.data_ptr())
        if li is not None:
            st = states[-4:][cur["state"]]
            kind = "delayed" if sa.untyped_storage().data_ptr() == st.scale.untyped_storage().data_ptr() else "exact"
            streams = range(cur["S"]) if cur["state"] == 3 else [cur["state"]]
            for s in streams:
                prev = last.get((s, li))
                trace.append((cur["step"], s, li, kind, None if prev is None else cur["step"] - prev))
                last[(s, li)] = cur["step"]
        return orig_gemm(Aq, sa, Wq, sw, C, **k)
    monkeypatch.setattr(eng, "forward", forward)
    monkeypatch.setattr(ops, "gemm_fp8", gemm_fp8)
    try:
        out = run()
    finally:
        model.step_hook = None
    return sorted(trace), out


@pytest.mark.parametrize("streams", [2, 3], ids=["t2i", "edit_3_streams"])
@pytest.mark.parametrize("taylor", [False, True], ids=["full_steps", "taylorseer"])
@pytest.mark.parametrize("batched", [True, False], ids=["cfg_batched", "cfg_sequential"])
@pytest.mark.parametrize("interval", [[0.0, 1.0], [0.4, 1.0]], ids=["cfg_everywhere", "cfg_off_late"])
def test_fp8_delayed_scale_schedule_matches_the_restatement(monkeypatch, interval, batched, taylor, streams):
    """10 Euler steps, timestep_shift 3, CFG text scale 4 (+ image scale 2 in the 3-stream form): the product's trace of exact / delayed down-projection
    inputs equals the oracle's under the same rule; every delayed use reads the maxima of the previous step (age 1); a step after TaylorSeer steps and
    the step where cfg_interval switches from the stream-batched state to the sequential one take the exact path."""
    from oracle import bagel_oracle as O
    from oracle import fp8 as F8
    mock_ops.install(monkeypatch)
    cfg = TINY_D128
    model = cpu_model(cfg)
    sizes = [(32, 32), (16, 48)]
    W, li, cache, ocache, kw, okw = _setup(model, cfg, sizes, streams)
    M1 = sum(int(x) for x in li["packed_seqlens"])
    gen = dict(num_timesteps=10, timestep_shift=3.0, cfg_text_scale=4.0, cfg_img_scale=2.0 if streams == 3 else 1.0, cfg_interval=interval,
               cfg_renorm_min=0.0, cfg_renorm_type="global" if streams == 2 else "text_channel", enable_taylorseer=taylor)
    model.gen_weight_quant, model.cfg_batched, model.fp8_delayed_scaling = "fp8", batched, True
    got, lat = _product_trace(monkeypatch, model, M1, lambda: model.generate_image(past_key_values=copy.deepcopy(cache), **kw, **gen, **li))
    assert all(torch.isfinite(x).all() for x in lat)
    O.FP8_WEIGHT_PTRS = O.fp8_gen_weight_ptrs(W)
    O.FP8_DELAYED = F8.DelayedScales(F8.down_proj_gen_ptrs(W))
    try:
        ref = O.generate_image(W, cfg, li, ocache, cfg_text=okw.get("cfg_text"), cfg_img=okw.get("cfg_img"), fp8_batched=batched,
                               **{k: v for k, v in gen.items() if k != "cfg_renorm_min"})
        want = sorted(O.FP8_DELAYED.trace)
    finally:
        O.FP8_WEIGHT_PTRS, O.FP8_DELAYED = set(), None
    L = cfg["llm"]["num_hidden_layers"]
    assert len(got) > 0 and any(k == "delayed" for _, _, _, k, _ in got)
    first_diff = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, f"product vs restatement from entry {first_diff}: {got[first_diff:first_diff + 2 * L]} vs {want[first_diff:first_diff + 2 * L]}"
    stale = [e for e in got if e[3] == "delayed" and e[4] != 1]
    assert not stale, f"delayed scales from rows older than the previous step: {stale}"
    if taylor:     # there were skipped steps, and the first full step after them re-measured its rows
        assert any(k == "exact" and age is not None and age > 1 for _, _, _, k, age in got)
    if interval[0] > 0 and batched:     # the first forward after the CFG switch runs on the sequential state: no history there
        ts, _ = model.flow_schedule(gen["num_timesteps"], gen["timestep_shift"])
        off = next(i for i, t in enumerate(ts.tolist()) if not t > interval[0])
        after = [s for s, *_ in got if s >= off]          # (with TaylorSeer the last steps may all be extrapolated)
        assert after or taylor
        assert all(k == "exact" for s, _, _, k, _ in got if after and s == min(after)), (off, after)
    assert all(torch.isfinite(x).all() for x in ref)
    for a, b in zip(lat, ref):
        assert a.shape == b.shape
