"""CPU: the attention probe's surface -- the symbol and its declaration, the argument checks of ops.attention_probe /
ops.self_attention_probe (all of them fire before a device is touched: every tensor here lives on the CPU), DreamVLA.token_groups
against the model's counters, ops.attention_mass / ops.patch_heat against the float64 restatement (tests/attention_probe_ref.py),
and the training-mode refusal.  The kernel itself: tests/test_attention_probe_gpu.py."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dreamvla_amd import _lib, ops
from dreamvla_amd.dreamvla_model import DreamVLA
from tests import attention_probe_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def test_symbol_is_bound_and_declared_and_abi_stays_9():
    assert "dvla_attn_probe" in _lib.SYMBOLS
    header = open(os.path.join(ROOT, "include", "dvla.h")).read()
    assert re.search(r"\bint\s+dvla_attn_probe\s*\(", header)
    assert re.search(r"#define\s+DVLA_ABI_VERSION\s+9\b", header) and _lib.ABI_VERSION == 9
    m = re.search(r"#define\s+DVLA_PROBE_MAX_ROWS\s+(\d+)", header)
    assert m and int(m.group(1)) == 32 == _lib.PROBE_MAX_ROWS == ops.PROBE_MAX_ROWS
    res, args = _lib.SYMBOLS["dvla_attn_probe"]
    assert len(args) == 9                      # params, rows, R, head_dim, Lk_full, per_head, out, workspace, stream
    assert os.path.exists(os.path.join(ROOT, "dreamvla_amd", "csrc", "attention_probe.hip"))


def _qk(B=2, Lq=5, Lk=7, H=2, D=64, dtype=BF):
    return torch.zeros(B, Lq, H, D, dtype=dtype), torch.zeros(B, Lk, H, D, dtype=dtype)


def _rows(B=2, R=3, dtype=torch.int32):
    return torch.zeros(B, R, dtype=dtype)


def _tables(Lq, Lk):
    vis = np.ones((Lq, Lk), dtype=bool)
    vis[:, 0] = False
    return ops.build_mask_tables(torch.where(torch.from_numpy(vis), 0.0, float("-inf")), device="cpu")


@pytest.mark.parametrize("what", ["q dtype", "k dtype", "q rank", "inner stride", "heads differ", "head_dim differ", "batch differ",
                                  "head_dim 4", "head_dim 136", "head_dim 20", "rows dtype", "rows rank", "rows batch", "R = 0", "R = 33",
                                  "mask Lq", "mask Lk", "mask type", "out shape", "out dtype", "cpu tensors"])
def test_every_argument_check_fires_before_a_device_is_touched(what):
    q, k = _qk()
    rows, kw = _rows(), dict(scale=0.125)
    if what == "q dtype":
        q = q.float()
    elif what == "k dtype":
        k = k.half()
    elif what == "q rank":
        q = q[0]
    elif what == "inner stride":
        k = torch.zeros(2, 7, 2, 128, dtype=BF)[..., ::2]
    elif what == "heads differ":
        k = torch.zeros(2, 7, 3, 64, dtype=BF)
    elif what == "head_dim differ":
        k = torch.zeros(2, 7, 2, 32, dtype=BF)
    elif what == "batch differ":
        k = torch.zeros(3, 7, 2, 64, dtype=BF)
    elif what.startswith("head_dim "):
        q, k = _qk(D=int(what.split()[1]))
    elif what == "rows dtype":
        rows = _rows(dtype=torch.int64)
    elif what == "rows rank":
        rows = torch.zeros(2, dtype=torch.int32)
    elif what == "rows batch":
        rows = _rows(B=3)
    elif what == "R = 0":
        rows = _rows(R=0)
    elif what == "R = 33":
        rows = _rows(R=33)
    elif what == "mask Lq":
        kw["mask_tables"] = _tables(6, 7)
    elif what == "mask Lk":
        kw["mask_tables"] = _tables(5, 8)
    elif what == "mask type":
        kw["mask_tables"] = torch.zeros(5, 7)
    elif what == "out shape":
        kw["out"] = torch.zeros(2, 3, 8)
    elif what == "out dtype":
        kw["out"] = torch.zeros(2, 3, 7, dtype=torch.float64)
    # ("cpu tensors": everything well-formed -- the device check is the last one and the only one left)
    with pytest.raises(ValueError):
        ops.attention_probe(q, k, rows, **kw)


def test_well_formed_masked_cpu_call_reaches_only_the_device_check():
    q, k = _qk()
    with pytest.raises(ValueError, match="GPU"):
        ops.attention_probe(q, k, _rows(), scale=0.125, mask_tables=_tables(5, 7), per_head=True)


@pytest.mark.parametrize("what", ["rank", "width", "dtype", "rows"])
def test_packed_probe_checks(what):
    qkv, rows, kw = torch.zeros(2, 5, 3 * 2 * 64, dtype=BF), _rows(), dict(num_heads=2)
    if what == "rank":
        qkv = qkv[0]
    elif what == "width":
        kw["num_heads"] = 3
    elif what == "dtype":
        qkv = qkv.to(torch.float16)
    elif what == "rows":
        rows = _rows(R=40)
    with pytest.raises(ValueError):
        ops.self_attention_probe(qkv, rows=rows, **kw)


def _counters(**kw):
    base = dict(NUM_RESAMPLER_QUERY=16, share_query=False, NUM_OBS_TOKEN=0, NUM_DEPTH_TOKEN=0, NUM_DINO_TOKEN=0, NUM_SAM_TOKEN=0,
                NUM_TRAJ_TOKEN=0, action_pred_steps=3)
    base.update(kw)
    return SimpleNamespace(**base)


def test_token_groups_follow_the_models_counters():
    # several dream heads, own queries each
    m = _counters(NUM_OBS_TOKEN=18, NUM_DEPTH_TOKEN=18, NUM_SAM_TOKEN=20, NUM_TRAJ_TOKEN=9)
    g = DreamVLA.token_groups(m)
    assert [n for n, _, _ in g] == ["text", "state", "image_primary", "image_wrist", "cls_primary", "cls_wrist", "dream_image",
                                    "dream_depth", "dream_sam", "dream_traj", "action"]
    assert g[2] == ("image_primary", 2, 16) and g[3] == ("image_wrist", 18, 16) and g[5] == ("cls_wrist", 35, 1)
    num_A = 1 + 1 + 2 * m.NUM_RESAMPLER_QUERY + 2                       # the mask rule's counters (DreamVLA._mask_rule)
    nq = 18 + 18 + 20 + 9
    assert g[6][1] == num_A and g[-1] == ("action", num_A + nq, 3)
    # the groups tile the block
    cur = 0
    for _, start, count in g:
        assert start == cur and count > 0
        cur += count
    assert cur == num_A + nq + 3
    # share_query: every head reads its columns of the same NUM_OBS_TOKEN rows -> one dream group
    m = _counters(share_query=True, NUM_OBS_TOKEN=18, NUM_DEPTH_TOKEN=18, NUM_DINO_TOKEN=18, NUM_RESAMPLER_QUERY=9)
    g = DreamVLA.token_groups(m)
    assert [n for n, _, _ in g][6:] == ["dream_shared", "action"]
    assert g[6] == ("dream_shared", 22, 18) and g[7] == ("action", 40, 3)
    # no dream head, no action queries
    g = DreamVLA.token_groups(_counters(action_pred_steps=0))
    assert [n for n, _, _ in g] == ["text", "state", "image_primary", "image_wrist", "cls_primary", "cls_wrist"]


def test_action_rows_are_built_from_test_select():
    m = _counters(NUM_OBS_TOKEN=18)
    blk = 36 + 18 + 3
    rows = DreamVLA._attention_rows(m, "action", 2, 4, torch.tensor([3, 0]), "cpu")
    assert rows.dtype == torch.int32 and rows.tolist() == [[3 * blk + 54, 3 * blk + 55, 3 * blk + 56], [54, 55, 56]]
    every = DreamVLA._attention_rows(m, "action", 2, 4, None, "cpu")
    assert every.shape == (2, 12) and every[1].tolist() == [s * blk + 54 + i for s in range(4) for i in range(3)]
    assert DreamVLA._attention_rows(m, "obs", 1, 4, torch.tensor([1]), "cpu").tolist() == [list(range(blk + 36, blk + 54))]
    with pytest.raises(ValueError):                       # 4 x 18 rows: more than the probe takes
        DreamVLA._attention_rows(m, "obs", 1, 4, None, "cpu")
    with pytest.raises(ValueError):
        DreamVLA._attention_rows(m, "wrist", 1, 4, None, "cpu")


def _stochastic(shape, gen, zero_rows=()):
    x = torch.rand(shape, generator=gen, dtype=torch.float64)
    x = x / x.sum(dim=-1, keepdim=True)
    for idx in zero_rows:
        x[idx] = 0.0
    return x


GROUPS = DreamVLA.token_groups(_counters(NUM_OBS_TOKEN=18, NUM_DEPTH_TOKEN=18, NUM_RESAMPLER_QUERY=4))


def test_attention_mass_against_the_restatement():
    gen = torch.Generator().manual_seed(3)
    S = 3
    blk = GROUPS[-1][1] + GROUPS[-1][2]
    maps = _stochastic((2, 2, 3, S * blk), gen, zero_rows=[(1, 0, 2)])
    got = ops.attention_mass(maps, GROUPS, S)
    assert got.shape == (2, 2, 3, S, len(GROUPS))
    np.testing.assert_allclose(got.numpy(), PR.attention_mass(maps.numpy(), GROUPS, S), rtol=1e-12, atol=1e-15)
    tot = got.sum(dim=(-1, -2))
    assert float(tot[1, 0, 2]) == 0.0                     # a row that sees nothing
    tot[1, 0, 2] = 1.0
    np.testing.assert_allclose(tot.numpy(), 1.0, rtol=1e-12)
    assert float(got[0, 0, 0, 0].sum()) > 0               # mass on the oldest window step is reported, not dropped
    with pytest.raises(ValueError):
        ops.attention_mass(maps, GROUPS, 4)


def test_patch_heat_against_the_restatement():
    gen = torch.Generator().manual_seed(4)
    B, S, n_lat, n_patch = 2, 3, 4, 9
    blk = GROUPS[-1][1] + GROUPS[-1][2]
    trunk = _stochastic((B, 2, 3, S * blk), gen)
    trunk[1, :, :, blk:] = 0.0                            # sequence 1 looks at the oldest window step only: no mass at position 2
    pos = torch.tensor([1, 2])
    for F in (1, S):
        res = _stochastic((2 * B * F, 3, n_lat, n_patch + n_lat), gen)
        got = ops.patch_heat(trunk, res, GROUPS, pos)
        assert got.shape == (B, 2, 3, 3)
        np.testing.assert_allclose(got.numpy(), PR.patch_heat(trunk.numpy(), res.numpy(), GROUPS, pos.tolist()), rtol=1e-10, atol=1e-15)
        np.testing.assert_allclose(got[0].sum(dim=(-1, -2)).numpy(), 1.0, rtol=1e-12)
        assert float(got[1].abs().max()) == 0.0           # mass 0 -> all zeros, not NaN
    roll = ops.attention_rollout(res[:1], n_patch)[0]
    np.testing.assert_allclose(roll.numpy(), PR.rollout(res[0].numpy(), n_patch), rtol=1e-12, atol=1e-15)
    with pytest.raises(ValueError):
        ops.patch_heat(trunk, res[:3], GROUPS, pos)


def test_a_probe_in_training_mode_raises():
    from dreamvla_amd.gpt2 import GPT2Config, GPT2Model
    from dreamvla_amd.perceiver_resampler import PerceiverResampler
    cfg = GPT2Config(hidden_size=64, n_layer=1, n_head=1, vocab_size=1)
    trunk = GPT2Model(cfg)
    probe = ops.AttentionProbe(torch.zeros(1, 1, dtype=torch.int32))
    assert trunk.training
    with pytest.raises(RuntimeError, match="eval"):
        trunk(inputs_embeds=torch.zeros(1, 4, 64), probe=probe)
    res = PerceiverResampler(dim=64, depth=1, num_latents=2)
    with pytest.raises(RuntimeError, match="eval"):
        res(torch.zeros(1, 1, 1, 3, 64), probe=ops.AttentionProbe())
    with pytest.raises(ValueError):
        ops.AttentionProbe(torch.zeros(1, 1, dtype=torch.int64))


def test_the_float64_restatement_itself():
    """softmax over the visible keys, exact zeros, head mean -- on a case small enough to write out"""
    q = np.zeros((1, 3, 2, 8))
    k = np.zeros((1, 4, 2, 8))
    q[0, :, :, 0] = 1.0
    k[0, :, 0, 0] = [0.0, np.log(2.0), np.log(3.0), 5.0]       # head 0: weights 1, 2, 3 on the visible keys
    vis = np.array([[1, 1, 1, 0], [0, 0, 0, 0], [1, 0, 0, 0]], dtype=bool)
    ref = PR.probabilities(q, k, [[0, 1, 2, 7]], 1.0, vis)
    np.testing.assert_allclose(ref["per_head"][0, 0, 0], [1 / 6, 2 / 6, 3 / 6, 0.0], rtol=1e-12)
    np.testing.assert_allclose(ref["per_head"][0, 1, 0], [1 / 3, 1 / 3, 1 / 3, 0.0], rtol=1e-12)
    np.testing.assert_allclose(ref["mean"][0, 0], [0.25, 1 / 3, 5 / 12, 0.0], rtol=1e-12)
    assert not ref["mean"][0, 1].any() and not ref["mean"][0, 3].any()     # blind row, row out of range
    assert ref["mean"][0, 2].tolist() == [1.0, 0.0, 0.0, 0.0]
    b = PR.bound(ref, 8, 4, per_head=False)
    assert b.shape == ref["mean"].shape and (b <= PR.issue_cap(ref["mean"])).all() and b[0, 0, 3] == 0.0
