"""GPU: attention maps through the model and the rollout engine (DreamVLA.decode_tokens / encode_frames(attention=...),
RolloutEngine(attention=...)) on a tiny random-init DreamVLA -- the small configuration of tests/rollout_checks.py with
atten_only_obs, no checkpoint, no reference files.

The maps are held to the float64 restatement (tests/attention_probe_ref.py) recomputed from what each layer's projection actually
produced (forward hooks on c_attn / to_q / to_kv) under the model's own mask, with the derived bound of that module; everything
else is exact: the action outputs with and without `attention`, the maps of the eager and the captured path, zero mass outside the
action rows' own window step."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import attention_probe_ref as PR

pytestmark = pytest.mark.gpu

DEV, BF = "cuda", torch.bfloat16
S, HID, HEADS, STEPS = 4, 512, 8, 3
BLK = 36 + 18 + STEPS


@functools.lru_cache(maxsize=None)
def _model(head):
    from dreamvla_amd.dreamvla_model import DreamVLA
    from oracle import weights
    torch.manual_seed(0)
    np.random.seed(0)
    m = DreamVLA(clip_device="cpu", vit_checkpoint_path=None, finetune_type="calvin", sequence_length=S, num_resampler_query=16,
                 num_obs_token_per_image=9, action_pred_steps=STEPS, transformer_layers=2, hidden_dim=HID, transformer_heads=HEADS,
                 phase="finetune", obs_pred=True, atten_only_obs=True, attn_robot_proprio_state=True, use_dit_head=(head == "dit"),
                 attn_implementation="sdpa")
    m.load_state_dict(weights.fill_state_dict(m.state_dict()), strict=True)
    m = m.to(BF).to(DEV)
    m._init_model_type()
    return m.eval()


def _hook(module, store):
    return module.register_forward_hook(lambda mod, args, out: store.append(out.detach().float().cpu()))


def _within_bound(tag, got, q, k, rows, scale, vis, Lk_axis):
    ref = PR.probabilities(q, k, rows, scale, vis)
    bnd = PR.bound(ref, q.shape[-1], Lk_axis, per_head=False)
    assert (bnd <= PR.issue_cap(ref["mean"])).all(), tag
    g = got.double().cpu().numpy()
    assert (g[ref["mean"] == 0.0] == 0.0).all(), tag
    err = np.abs(g - ref["mean"])
    print(tag, "worst err / bound", float((err[bnd > 0] / bnd[bnd > 0]).max()))
    assert (err <= bnd).all(), (tag, float(err.max()))


def test_decode_tokens_maps_against_float64_and_actions_unchanged():
    from dreamvla_amd import ops
    m = _model("mlp")
    B = 2
    g = torch.Generator().manual_seed(1)
    parts = torch.randn(B, S, 36, HID, generator=g).to(BF).to(DEV)
    sel = torch.tensor([3, 1], device=DEV)
    store = []
    hooks = [_hook(blk.attn.c_attn, store) for blk in m.transformer_backbone.h]
    with torch.no_grad():
        with_maps = m.decode_tokens(parts, mode="test", test_select=sel, attention=dict(rows="action", layers="all"))
    for h in hooks:
        h.remove()
    maps = m.last_attention["trunk"]
    with torch.no_grad():
        plain = m.decode_tokens(parts, mode="test", test_select=sel)
    assert torch.equal(with_maps[0], plain[0]) and torch.equal(with_maps[1], plain[1])
    L = S * BLK
    assert maps.shape == (B, 2, STEPS, L) and maps.dtype == torch.float32 and len(store) == 2
    rows = np.array([[p * BLK + 54 + i for i in range(STEPS)] for p in (3, 1)], dtype=np.int32)
    vis = (m.attention_mask == 0).cpu().numpy()
    mt = ops.mask_tables_for(m.attention_mask)
    for layer, qkv in enumerate(store):
        v5 = qkv.view(B, L, 3, HEADS, 64).numpy()
        _within_bound(f"trunk layer {layer}", maps[:, layer], v5[:, :, 0], v5[:, :, 1], rows, 1.0 / math.sqrt(64), vis, mt.Lk)
    # under atten_only_obs an action row reads its own window step only
    for b, p in enumerate((3, 1)):
        other = torch.ones(L, dtype=torch.bool, device=DEV)
        other[p * BLK:(p + 1) * BLK] = False
        assert float(maps[b][..., other].abs().max()) == 0.0
    # other specs: the last layer, the dream queries; every position without test_select
    with torch.no_grad():
        m.decode_tokens(parts, mode="test", test_select=sel, attention=dict(rows="obs", layers="last"))
    last = m.last_attention["trunk"]
    assert last.shape == (B, 1, 18, L)
    with torch.no_grad():
        m.decode_tokens(parts, mode="test", attention=dict(rows="action", layers=[1]))
    every = m.last_attention["trunk"]
    assert every.shape == (B, 1, S * STEPS, L)
    assert torch.equal(every[0, 0, 3 * STEPS:4 * STEPS], maps[0, 1]) and torch.equal(every[1, 0, STEPS:2 * STEPS], maps[1, 1])
    with pytest.raises(ValueError):
        m.decode_tokens(parts, mode="train", attention=dict(rows="action"))
    with pytest.raises(ValueError):
        m.decode_tokens(parts, mode="test", attention=dict(rows="obs"))            # 4 x 18 rows


def test_dit_head_actions_do_not_depend_on_attention():
    m = _model("dit")
    B = 2
    g = torch.Generator().manual_seed(2)
    parts = torch.randn(B, S, 36, HID, generator=g).to(BF).to(DEV)
    sel = torch.tensor([0, 2], device=DEV)
    noise = torch.randn(B, STEPS, 7, generator=g).to(DEV)
    with torch.no_grad():
        a = m.decode_tokens(parts, mode="test", test_select=sel, test_noise=noise, attention=dict(rows="action", layers="last"))
        b = m.decode_tokens(parts, mode="test", test_select=sel, test_noise=noise)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert m.last_attention["trunk"].shape == (B, 1, STEPS, S * BLK)


def test_encode_frames_resampler_maps():
    m = _model("mlp")
    B, F = 1, 2
    g = torch.Generator().manual_seed(3)
    ip, iw = (torch.randn(B, F, 3, 224, 224, generator=g).to(BF).to(DEV) for _ in range(2))
    st = torch.cat([torch.rand(B, F, 6, generator=g), torch.ones(B, F, 1)], -1).to(BF).to(DEV)
    text = torch.zeros(B, F, 1, HID, dtype=BF, device=DEV)
    qs, kvs = [], []
    hooks = [_hook(layer[0].to_q, qs) for layer in m.perceiver_resampler.layers]
    hooks += [_hook(layer[0].to_kv, kvs) for layer in m.perceiver_resampler.layers]
    with torch.no_grad():
        with_maps = m.encode_frames(ip, iw, st, None, text_embedding=text, attention=dict(rows="action"))
    for h in hooks:
        h.remove()
    res = m.last_attention["resampler"]
    with torch.no_grad():
        plain = m.encode_frames(ip, iw, st, None, text_embedding=text)
    assert all(torch.equal(a, b) for a, b in zip(with_maps, plain))
    n, depth = 2 * B * F, len(m.perceiver_resampler.layers)
    assert res.shape == (n, depth, 16, 196 + 16) and res.dtype == torch.float32
    rows = np.tile(np.arange(16, dtype=np.int32), (n, 1))
    for layer in range(depth):
        q = qs[layer].view(n, 16, 8, 64).numpy()
        k = kvs[layer].view(n, 212, 2, 8, 64)[:, :, 0].numpy()
        _within_bound(f"resampler layer {layer}", res[:, layer], q, k, rows, 64 ** -0.5, None, 212)


def _frames(B, gen):
    return (torch.randn(B, 3, 224, 224, generator=gen).to(BF), torch.randn(B, 3, 224, 224, generator=gen).to(BF),
            torch.cat([torch.rand(B, 6, generator=gen), (torch.rand(B, 1, generator=gen) > 0.5).float()], -1).to(BF))


def _text(B):
    t = torch.zeros(B, 77, dtype=torch.long)
    t[:, 0], t[:, 1:5], t[:, 5] = 49406, 1000, 49407
    return t


def _rollout(head, B, use_graph, attention, sample="newest", steps=5, reset_at=3):
    """-> per step (action, arm, gripper, last_attention, executed positions)"""
    from dreamvla_amd.rollout import RolloutEngine
    m = _model(head)
    eng = RolloutEngine(m, B, use_graph=use_graph, warmup_decodes=2, sample=sample, attention=attention)
    g = torch.Generator().manual_seed(7)
    text, out = _text(B), []
    for t in range(steps):
        if t == reset_at and B > 1:                        # episode 1 starts again next to two full histories
            eng.reset(torch.tensor([b == 1 for b in range(B)]))
        ip, iw, st = _frames(B, g)
        noise = torch.randn(B * S, STEPS, 7, generator=g).to(DEV) if head == "dit" else None
        action, arm, grip = eng.step(ip, iw, st, text, noise=noise)
        out.append((action.clone(), arm.clone(), grip.clone(), dict(eng.last_attention), (eng.count - 1).clone()))
    if use_graph:
        assert eng.graphs_captured
    return out


SPEC = dict(rows="action", layers="all")


def test_engine_maps_on_the_eager_and_the_graph_path():
    B = 3
    runs = {(gr, att is not None): _rollout("mlp", B, gr, att) for gr in (False, True) for att in (None, SPEC)}
    L = S * BLK
    for t in range(5):
        for gr in (False, True):                           # actions: bit-identical with and without attention
            for i in range(3):
                assert torch.equal(runs[(gr, True)][t][i], runs[(gr, False)][t][i]), (t, gr, i)
        assert runs[(True, False)][t][3] == {}
        e, g = runs[(False, True)][t][3], runs[(True, True)][t][3]
        pos = runs[(True, True)][t][4]
        if t >= 3:
            assert pos.tolist() == [3, t - 3, 3]           # a fresh reset next to full histories
        assert e["groups"] == g["groups"] and e["groups"][-1] == "action" and "image_wrist" in e["groups"]
        for key, shape in (("trunk", (B, 2, STEPS, L)), ("mass", (B, STEPS, S, len(e["groups"]))), ("heat", (B, 2, 14, 14)),
                           ("resampler", (2 * B, 3, 16, 212))):
            assert g[key].shape == shape and g[key].dtype == torch.float32, key
            assert torch.equal(e[key], g[key]), (t, key)   # the captured graph computes what the eager path computes
        mass, heat = g["mass"], g["heat"]
        assert torch.allclose(mass.sum(dim=(-1, -2)), torch.ones(B, STEPS, device=DEV), atol=1e-5)
        assert torch.allclose(heat.sum(dim=(-1, -2)), torch.ones(B, 2, device=DEV), atol=1e-5) and bool((heat >= 0).all())
        for b in range(B):                                 # atten_only_obs: nothing outside the executed window step
            other = torch.ones(S, dtype=torch.bool)
            other[int(pos[b])] = False
            assert float(mass[b][:, other.to(DEV)].abs().max()) == 0.0
            assert float(mass[b][:, int(pos[b])].sum()) > 0


@pytest.mark.parametrize("use_graph,sample", [(True, "newest"), (False, "all")])
def test_engine_dit_head_single_episode(use_graph, sample):
    """one episode with the DiT head (the one-XCD sampler kernel where the device allows it), and sample="all": same actions with
    and without attention, maps of the executed position, a short padded history at the first steps"""
    a = _rollout("dit", 1, use_graph, SPEC, sample=sample, steps=4)
    b = _rollout("dit", 1, use_graph, None, sample=sample, steps=4)
    for t in range(4):
        for i in range(3):
            assert torch.equal(a[t][i], b[t][i]), (t, i)
        att, pos = a[t][3], int(a[t][4][0])
        assert pos == min(t, S - 1) and att["trunk"].shape == (1, 2, STEPS, S * BLK)
        other = torch.ones(S, dtype=torch.bool)
        other[pos] = False
        assert float(att["mass"][0][:, other.to(DEV)].abs().max()) == 0.0
        assert torch.allclose(att["mass"].sum(dim=(-1, -2)), torch.ones(1, STEPS, device=DEV), atol=1e-5)
