"""GPU: DeviceCollator(device_labels=True) -- depth, DINO, SAM and track labels built on the device -- against the default collator.

The contract: every entry e of the 13-tuple equals the default collator's `e.to("cuda", label_dtype)` bit for bit, the entries of
the track dictionary the default's `.to("cuda")` (dtype kept: the flow mask thresholds the tracks at 1 px); entries that are no
labels (cameras, text, actions, states, robot_obs) are what they are today.  The depth path is two gathers and one rounding, the
feature path a copy and one rounding, so every comparison is equality of bit patterns.  Both collators draw their shifts from
generators seeded alike; afterwards the generators must stand at the same point of their streams."""
import numpy as np
import pytest
import torch

from tests.collate_samples import fake_tokenize, make_samples
from tests.depth_cases import bits

BF = torch.bfloat16
LABELS = {6: "depth_static", 7: "depth_gripper", 8: "dino", 9: "dino_gripper", 10: "sam", 11: "sam_gripper"}
TRACK_KEYS = ("tracks", "track_visibility", "tracks_gripper", "track_visibility_gripper")


def _case(name, dataset="calvin", act_step=1, T=5):
    return dict(name=name, dataset=dataset, T=T, act_step=act_step, extras=("sam", "dino", "track"))


def _collator(case, seed, device_labels, traj_cons=False, label_dtype=BF, **kw):
    from dreamvla_amd import collate
    cls = collate.LiberoDeviceCollator if case["dataset"] == "libero" else collate.DeviceCollator
    g = torch.Generator().manual_seed(seed)
    col = cls(fake_tokenize, window_size=case["T"] - case["act_step"] + 1, rgb_pad=kw.pop("rgb_pad", 10), gripper_pad=kw.pop("gripper_pad", 4),
              traj_cons=traj_cons, act_step=case["act_step"], load_track_labels=True, device="cuda", generator=g,
              device_labels=device_labels, label_dtype=label_dtype, **kw)
    return col, g


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.device == b.device and torch.equal(bits(a) if a.is_floating_point() else a,
                                                                                               bits(b) if b.is_floating_point() else b)


def _assert_contract(got, ref, label_dtype=BF, depth=True):
    assert len(got) == len(ref) == 13
    for e in (0, 3):                                                    # the cameras: device tensors either way
        assert _same_bits(got[e], ref[e]), e
    for e in (1, 2, 4, 5):                                              # no labels: host tensors, unchanged
        assert not got[e].is_cuda and _same_bits(got[e], ref[e]), e
    for e, name in LABELS.items():
        if not depth and e in (6, 7):
            assert got[e] is None and ref[e] is None
            continue
        assert got[e].is_cuda and got[e].dtype == label_dtype, name
        assert _same_bits(got[e], ref[e].to("cuda", label_dtype)), name
    assert set(got[12]) == set(ref[12]) == set(TRACK_KEYS)
    for k in TRACK_KEYS:
        assert got[12][k].is_cuda and _same_bits(got[12][k], ref[12][k].to("cuda")), k


@pytest.mark.gpu
@pytest.mark.parametrize("act_step", [1, 3])
@pytest.mark.parametrize("traj_cons", [False, True], ids=["forward", "traj_cons"])
def test_device_labels_equal_the_default_collator(traj_cons, act_step):
    case = _case(f"labels_a{act_step}", act_step=act_step)
    new, g_new = _collator(case, 5, True, traj_cons)
    old, g_old = _collator(case, 5, False, traj_cons)
    got, ref = new(make_samples(case)), old(make_samples(case))
    assert ref[6].dtype == torch.float32 and not ref[6].is_cuda         # the default is what it was: host fp32 labels
    assert got[6].shape == (2, case["T"] - act_step + 1, 1, 224, 224)
    _assert_contract(got, ref)
    assert torch.equal(torch.randint(0, 1 << 30, (8,), generator=g_new), torch.randint(0, 1 << 30, (8,), generator=g_old))
    if traj_cons:                                                       # the depth maps were shifted by their own draw
        plain, _ = _collator(case, 5, True, False)
        assert not torch.equal(bits(plain(make_samples(case))[6]), bits(got[6]))


@pytest.mark.gpu
def test_fp32_labels_and_no_shift():
    case = _case("labels_f32")
    new, _ = _collator(case, 6, True, True, torch.float32, rgb_pad=-1)
    old, _ = _collator(case, 6, False, True, rgb_pad=-1)
    _assert_contract(new(make_samples(case)), old(make_samples(case)), torch.float32)


@pytest.mark.gpu
def test_libero_has_no_depth_and_returns_device_tracks():
    case = _case("labels_libero", dataset="libero")
    new, g_new = _collator(case, 7, True, True)
    old, g_old = _collator(case, 7, False, True)
    got, ref = new(make_samples(case)), old(make_samples(case))
    assert got[6] is None and got[7] is None
    _assert_contract(got, ref, depth=False)
    assert torch.equal(torch.randint(0, 1 << 30, (8,), generator=g_new), torch.randint(0, 1 << 30, (8,), generator=g_old))


@pytest.mark.gpu
def test_two_depth_sizes_in_a_batch_are_refused():
    case = _case("labels_sizes")
    smp = make_samples(case)
    smp[1]["depth_obs"]["depth_static"][2] = smp[1]["depth_obs"]["depth_gripper"][0]          # an 84 x 84 map among 200 x 200 ones
    new, _ = _collator(case, 8, True)
    with pytest.raises(ValueError, match="must have one size"):
        new(smp)


@pytest.mark.gpu
def test_two_calls_without_a_synchronise_in_between():
    """different samples, back to back, nothing waited for: a staging buffer rewritten under the first call's copies would show
    in the first result"""
    a, b = _case("labels_first"), _case("labels_second")
    new, _ = _collator(a, 9, True, True)
    old, _ = _collator(a, 9, False, True)
    sa, sb = make_samples(a), make_samples(b)
    assert not np.array_equal(sa[0]["depth_obs"]["depth_static"][0], sb[0]["depth_obs"]["depth_static"][0])
    got_a = new(sa)
    got_b = new(sb)
    ref_a, ref_b = old(make_samples(a)), old(make_samples(b))
    _assert_contract(got_a, ref_a)
    _assert_contract(got_b, ref_b)


@pytest.mark.gpu
def test_fused_losses_take_the_labels_as_they_come():
    """losses.calvin_losses(fused=True) on the new collator's entries with no `.to` in between: the same bits as on the default
    collator's labels moved by hand.  Feature rows of 64 columns (the cosine kernel's vector width) replace the samples' 8 / 6."""
    from dreamvla_amd import losses
    S, fut = 2, 3
    case = _case("labels_loss", T=S + fut)
    g = torch.Generator().manual_seed(21)

    def samples():
        smp = make_samples(case)
        gg = torch.Generator().manual_seed(22)
        for s in smp:
            s["dino_features_obs"] = {k: torch.randn(case["T"], 16, 64, generator=gg) for k in ("dino_feats_static", "dino_feats_gripper")}
            s["sam_features_obs"] = {k: torch.randn(case["T"], 16, 128, generator=gg) for k in ("sam_feats_static", "sam_feats_gripper")}
        return smp
    new, _ = _collator(case, 10, True, True)
    old, _ = _collator(case, 10, False, True)
    got, ref = new(samples()), old(samples())
    bs = 2
    keys = {0: "image_primary", 3: "image_wrist", 6: "depth_primary", 7: "depth_wrist", 8: "dino_primary", 9: "dino_wrist",
            10: "sam_primary", 11: "sam_wrist"}
    batch_new = {k: got[e] for e, k in keys.items()}
    batch_ref = {k: ref[e].to("cuda", BF) for e, k in keys.items()}
    depth_pred = (torch.rand(bs * S, 2, 1, 196, 256, generator=g) * 4 + 0.1).to("cuda", BF)
    dino_pred = torch.randn(bs * S, 2, 1, 16, 64, generator=g).to("cuda", BF)
    sam_pred = torch.randn(bs * S, 2, 1, 16, 128, generator=g).to("cuda", BF)
    arm = torch.zeros((), device="cuda")
    out = (arm, arm, None, None, None, None, depth_pred, None, dino_pred, sam_pred)
    _, parts_new = losses.calvin_losses(out, batch_new, sequence_length=S, future_steps=fut, fused=True)
    _, parts_ref = losses.calvin_losses(out, batch_ref, sequence_length=S, future_steps=fut, fused=True)
    for k in ("depth", "dino", "sam"):
        assert torch.isfinite(parts_new[k]) and float(parts_new[k]) != 0.0, k
        assert torch.equal(parts_new[k], parts_ref[k]), (k, float(parts_new[k]), float(parts_ref[k]))
