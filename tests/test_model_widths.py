"""CPU: models of width other than 1024 (fixtures W and V of tests/make_golden_widths.py, from the REAL reference).

W = the reference's own CLI defaults (hidden_dim 384, 12 heads, 12 layers): trunk head_dim 32, dream-head decoders 384 / 16 = 24.
V = hidden_dim 768, 12 heads, LIBERO flags with the dino / sam / trajectory heads: trunk head_dim 64, decoders 768 / 16 = 48.
The HIP model constructs with the reference's state_dict surface, and the oracle (which the GPU checks compare the kernels
against) reproduces the reference's outputs and gradients."""
import json
import math
import os

import pytest
import torch

from oracle import model_ref as M
from tests import model_checks as C

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _surface(name):
    return json.load(open(os.path.join(GOLD, f"state_dict_surface_{name}.json")))


@pytest.mark.parametrize("name", ["W", "V"])
def test_hip_model_constructs_with_the_reference_surface(name):
    from dreamvla_amd.dreamvla_model import DreamVLA
    surf = _surface(name)
    assert surf["cfg"] == C.load(f"dreamvla_{name}.pt")["cfg"]
    m = DreamVLA(clip_device="cpu", vit_checkpoint_path=None, **surf["cfg"])
    mine = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert set(mine) == set(surf["entries"]), sorted(set(mine) ^ set(surf["entries"]))[:10]
    bad = [k for k in mine if mine[k] != surf["entries"][k]]
    assert not bad, bad[:10]
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == surf["trainable"]
    trunk = m.transformer_backbone.h[0].attn
    assert trunk.head_dim == surf["cfg"]["hidden_dim"] // surf["cfg"]["transformer_heads"]


@pytest.mark.parametrize("name", ["W", "V"])
def test_oracle_full_model_vs_golden(name):
    fx = C.load(f"dreamvla_{name}.pt")
    cfg = fx["cfg"]
    m = C.build_hip_model(cfg)
    sd = C.f32(m.state_dict())
    inp = C.golden_inputs(fx)
    with torch.no_grad():
        out = M.dreamvla_forward(sd, cfg, inp["image_primary"], inp["image_wrist"], inp["state"], inp["text_token"],
                                 action_label=fx["action_label"], mode="train", dit_noise=fx.get("dit_noise"),
                                 dit_timestep=fx.get("dit_timestep"))
    for r in C.compare_outputs(out, fx["train"], 5e-5, f"oracle.{name}.train"):
        assert r["ok"], r
    with torch.no_grad():
        out = M.dreamvla_forward(sd, cfg, inp["image_primary"], inp["image_wrist"], inp["state"], inp["text_token"],
                                 mode="test", dit_noise=fx["test_noise"])
    for r in C.compare_outputs(out, fx["test"], 5e-5, f"oracle.{name}.test"):
        assert r["ok"], r


@pytest.mark.parametrize("name", ["V", "W"])
def test_oracle_autograd_vs_reference_gradients(name):
    fx = C.load(f"dreamvla_{name}.pt")
    gall = C.load(f"grads_{name}.pt")
    gfx = gall["entries"]
    m = C.build_hip_model(fx["cfg"])
    grads, _, _ = C.oracle_grads(fx, C.f32(m.state_dict()))
    assert len(gfx) > 50
    for k, e in gfx.items():
        assert k in grads, f"oracle produced no gradient for {k}"
        g = grads[k].flatten()
        n = float(g.norm())
        assert abs(n - e["norm"]) <= 2e-4 * e["norm"] + 1e-9, (k, n, e["norm"])
        off, cnt = e["sample"]          # strided samples, stored flat for all tensors (tests/make_golden_widths.py)
        idx, vals = gall["sample_idx"][off:off + cnt], gall["sample_vals"][off:off + cnt]
        d = float((g[idx] - vals).norm() / max(float(vals.norm()), 1e-12 * e["norm"] + 1e-30))
        assert d <= 3e-3 or float((g[idx] - vals).abs().max()) <= 1e-5 * e["absmax"], (k, d)


@pytest.mark.parametrize("hidden, heads", [(384, 12), (512, 16), (768, 16), (1536, 12)])
def test_trunk_builds_at_supported_head_widths(hidden, heads):
    from dreamvla_amd.gpt2 import GPT2Attention, GPT2Config
    cfg = GPT2Config(hidden_size=hidden, n_head=heads, n_layer=1)
    a = GPT2Attention(cfg)
    assert a.head_dim == hidden // heads


@pytest.mark.parametrize("hidden, heads", [(360, 12), (2176, 16), (100, 3)])
def test_trunk_refuses_unsupported_head_widths_and_names_the_set(hidden, heads):
    from dreamvla_amd.gpt2 import GPT2Attention, GPT2Config
    with pytest.raises(ValueError, match="multiple of 8 from 8 to 128"):
        GPT2Attention(GPT2Config(hidden_size=hidden, n_head=heads, n_layer=1))


def _route(monkeypatch, B, L, D, H=2, mask_tables=None, dropout_p=0.0):
    """which autograd Function ops.self_attention hands a (B, L, 3 H D) problem to, and the head_dim it hands over -- both
    Functions take (qkv, heads, head_dim, ...); _SelfAttention with 64 is the MFMA kernel family, with any other width the
    head-width-generic one (test_raw_launchers_pick_the_kernel_family_from_head_dim below).  No kernel runs."""
    from dreamvla_amd import ops
    seen = []
    for name in ("_SelfAttention", "_SelfAttentionSmall"):
        monkeypatch.setattr(getattr(ops, name), "apply", staticmethod(lambda *a, _n=name: seen.append((_n, a[2]))))
    monkeypatch.setattr(ops, "to_compute", lambda x: x)
    ops.self_attention(torch.zeros(B, L, 3 * H * D, dtype=torch.bfloat16), H, scale=1.0 / math.sqrt(D),
                       mask_tables=mask_tables, dropout_p=dropout_p, head_dim=D)
    return seen


def test_routing_keeps_head_width_64_and_the_short_kernel(monkeypatch):
    assert _route(monkeypatch, 2, 205, 64) == [("_SelfAttention", 64)]
    assert _route(monkeypatch, 1792, 6, 96) == [("_SelfAttentionSmall", 96)]   # DiT-S: unchanged
    assert _route(monkeypatch, 4, 64, 24) == [("_SelfAttentionSmall", 24)]


def test_routing_sends_what_raised_before_to_the_generic_kernels(monkeypatch):
    assert _route(monkeypatch, 1, 205, 24) == [("_SelfAttention", 24)]         # W decoder
    assert _route(monkeypatch, 1, 265, 48) == [("_SelfAttention", 48)]         # V decoder
    assert _route(monkeypatch, 1, 40, 32, dropout_p=0.1) == [("_SelfAttention", 32)]
    assert _route(monkeypatch, 1, 64, 128) == [("_SelfAttention", 128)]        # over the short kernel's LDS
    assert _route(monkeypatch, 1, 40, 32, mask_tables=object()) == [("_SelfAttention", 32)]


def test_raw_launchers_pick_the_kernel_family_from_head_dim(monkeypatch):
    """attn_fwd_raw / attn_bwd_raw: dvla_attn_fwd / _bwd for head_dim 64 only, dvla_attn_hd_fwd / _bwd (with the width) for every
    other -- what makes the head_dim of _route the kernel family.  Library, tensor checks and parameter block are stubs."""
    from dreamvla_amd import _lib, ops
    calls = []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, a[1] if len(a) == 3 else None)) or 0

    monkeypatch.setattr(_lib, "load", lambda: Lib())
    monkeypatch.setattr(ops, "_req", lambda t, *a, **k: t)
    monkeypatch.setattr(ops, "_attn_params", lambda *a, **k: _lib.AttnParams())
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    for D in (8, 24, 32, 48, 56, 64, 72, 96, 128):
        q = torch.zeros(1, 5, 2, D, dtype=torch.bfloat16)
        del calls[:]
        o, lse = ops.attn_fwd_raw(q, q, q, scale=1.0, head_dim=D)
        ops.attn_bwd_raw(q, q, q, o, lse, o, *(torch.empty_like(q) for _ in range(3)), scale=1.0, head_dim=D)
        assert calls == ([("dvla_attn_fwd", None), ("dvla_attn_bwd", None)] if D == 64 else
                         [("dvla_attn_hd_fwd", D), ("dvla_attn_hd_bwd", D)]), (D, calls)


@pytest.mark.parametrize("D", [12, 136])
def test_routing_refuses_unsupported_head_widths(monkeypatch, D):
    from dreamvla_amd._lib import DvlaError
    with pytest.raises(DvlaError, match="multiples of 8"):
        _route(monkeypatch, 1, 205, D)
